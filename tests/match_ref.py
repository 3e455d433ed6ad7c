"""Reference for sh_match (tests/test_match_ref.py pins it, tests/test_match_gpu.py compares the engine with it), pure
numpy and Python: the edge list and k() are msf_ref's (the graph rule is the same), mkeys() is MKEY of the header,
greedy() the serial definition -- the edges in ascending MKEY, each kept when both its ends are still free --, rounds() a
simulator of the rounds of csrc/match.hip.h that returns what the device reports per round, certify() a check of a mate
vector that needs no gold, and the makers of the patterns the GPU tests run on."""
import numpy as np

import msf_ref as F
import wcc_ref as W
from color_ref import mix32

MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def unmix32(y):
    """The inverse of mix32 on one word (every step of mix32 is a bijection of the 32-bit words)."""
    m = 0xFFFFFFFF
    y = int(y) & m
    y ^= y >> 16
    y = (y * pow(0x846CA68B, -1, 1 << 32)) & m
    y ^= (y >> 15) ^ (y >> 30)
    y = (y * pow(0x7FEB352D, -1, 1 << 32)) & m
    y ^= y >> 16
    return y


def mkeys(k, heavy, seed):
    """MKEY(e) = hi << 32 | lo (uint64): hi = k for heavy == 0, ~k for heavy == 1; lo = e for seed == 0, else
    mix32(e ^ seed)."""
    assert heavy in (0, 1)
    k = np.asarray(k, np.uint32)
    hi = (~k if heavy else k).astype(np.uint64)
    e = np.arange(len(k), dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFF
    lo = e if seed == 0 else mix32(e ^ np.uint64(seed)).astype(np.uint64)
    return (hi << np.uint64(32)) | lo


def greedy(n, eu, ev, keys):
    """-> (mate, in_match): the serial definition."""
    mate = np.full(n, -1, np.int32)
    chosen = np.zeros(len(eu), np.int32)
    for e in np.argsort(np.asarray(keys, np.uint64), kind="stable").tolist():
        u, v = int(eu[e]), int(ev[e])
        if mate[u] < 0 and mate[v] < 0:
            mate[u], mate[v], chosen[e] = v, u, 1
    return mate, chosen


def rounds(n, eu, ev, keys, max_rounds=1 << 30):
    """The rounds of match.hip.h on one state per launch: drop the listed edges with a matched end, the kept ones bid
    for both ends, the kept edges that hold both their ends' words are matched.  -> dict(mate, in_match, rounds, complete,
    walked, kept, matched, pairs)."""
    eu, ev, keys = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(keys, np.uint64)
    mate = np.full(n, -1, np.int32)
    chosen = np.zeros(len(eu), np.int32)
    lst = np.arange(len(eu), dtype=np.int64)
    walked, kept, matched, complete = [], [], [], n == 0
    while n > 0 and len(walked) < max_rounds:
        walked.append(len(lst))
        lst = lst[(mate[eu[lst]] < 0) & (mate[ev[lst]] < 0)]
        kept.append(len(lst))
        if len(lst) == 0:
            matched.append(0)
            complete = True
            break
        best = np.full(n, MAX, np.uint64)
        np.minimum.at(best, eu[lst], keys[lst])
        np.minimum.at(best, ev[lst], keys[lst])
        hit = lst[(best[eu[lst]] == keys[lst]) & (best[ev[lst]] == keys[lst])]
        mate[eu[hit]] = ev[hit]
        mate[ev[hit]] = eu[hit]
        chosen[hit] = 1
        matched.append(len(hit))
    return dict(mate=mate, in_match=chosen, rounds=len(walked), complete=complete, walked=np.array(walked, np.int64),
                kept=np.array(kept, np.int64), matched=np.array(matched, np.int64), pairs=int(chosen.sum()))


def certify(mate, eu, ev, keys):
    """'' when mate is the greedy matching of the edges under the keys, else what is wrong.  Needs no gold: (1) mate is an
    involution over existing edges; (2) no edge has two free ends; (3) every unmatched edge touches a matched edge with a
    smaller key.  (A maximal matching with (3) is greedy's: take the unmatched edge of smallest key that greedy takes, or
    the matched one of smallest key that greedy does not take; either contradicts (3) or the keys below it.)"""
    mate = np.asarray(mate, np.int64)
    eu, ev, keys = np.asarray(eu, np.int64), np.asarray(ev, np.int64), np.asarray(keys, np.uint64)
    n = len(mate)
    v = np.arange(n, dtype=np.int64)
    if np.any((mate < -1) | (mate >= n)):
        return "a mate outside [-1, rows)"
    on = mate >= 0
    if np.any(mate[mate[on]] != v[on]) or np.any(mate[on] == v[on]):
        return "mate is no involution"
    is_matched = mate[eu] == ev
    if int(is_matched.sum()) * 2 != int(on.sum()):
        return "a pair that is no edge"
    if np.any((mate[eu] < 0) & (mate[ev] < 0)):
        return "an edge with two free ends"
    key_at = np.full(n, MAX, np.uint64)   # the key of the matched edge at v
    key_at[eu[is_matched]] = keys[is_matched]
    key_at[ev[is_matched]] = keys[is_matched]
    rest = ~is_matched
    if np.any(np.minimum(key_at[eu[rest]], key_at[ev[rest]]) >= keys[rest]):
        return "an unmatched edge below both matched edges it touches"
    return ""


def case(mat, heavy, seed):
    """-> (n, eu, ev, weight, keys) of a matrix under an order."""
    eu, ev, weight, k = F.edges(*mat)
    return mat[0], eu, ev, weight, mkeys(k, heavy, seed)


# ---- the patterns
def ascending_path(n=60):
    """The path 0 - 1 - ... - (n - 1) whose edge i weighs i + 1: under heavy == 0 and seed == 0 the keys ascend along it,
    and every round matches the first kept edge alone."""
    return F.by_edge(W.path(n), np.arange(1, n, dtype=np.float32))


def stars_and_path(edges):
    """Exactly `edges` edges without a perfect matching: stars of 9 leaves (hub first) as long as 9 edges fit, the rest a
    path; drawn weights.  Every star loses 8 edges to its first pair, so kept differs from walked."""
    src, dst, base, left = [], [], 0, edges
    while left >= 9 + 3:
        src.append(np.full(9, base, np.int64))
        dst.append(base + 1 + np.arange(9, dtype=np.int64))
        base, left = base + 10, left - 9
    src.append(base + np.arange(left, dtype=np.int64))
    dst.append(base + 1 + np.arange(left, dtype=np.int64))
    mat = W.csr(base + left + 1, np.concatenate(src), np.concatenate(dst))
    return F.weighted(mat, "drawn", seed=edges)


def hub(k=70_001):
    """A hub (vertex 0) with k leaves, drawn weights: one best word wanted by every edge."""
    return F.hub(k)


def packed4(weights):
    """Every graph on 4 labelled vertices, block-diagonally in one matrix (graph g on the vertices 4g .. 4g + 3), both
    directions stored; weights "equal", "ascending" or "descending" in the edge id of the union."""
    pairs = [(u, v) for u in range(4) for v in range(u + 1, 4)]
    src, dst = [], []
    for mask in range(64):
        for i, (u, v) in enumerate(pairs):
            if mask >> i & 1:
                src.append(4 * mask + u)
                dst.append(4 * mask + v)
    src, dst = np.array(src, np.int64), np.array(dst, np.int64)
    mat = W.csr(256, np.concatenate([src, dst]), np.concatenate([dst, src]))
    m = len(src)
    w = {"equal": np.ones(m), "ascending": np.arange(1, m + 1), "descending": np.arange(m, 0, -1)}[weights]
    return F.by_edge(mat, w.astype(np.float32))
