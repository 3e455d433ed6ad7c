"""Reference for sh_msf (tests/test_msf_ref.py pins it, tests/test_msf_gpu.py compares the engine with it), pure numpy and
Python: edges() is the edge list and the weights by the rules of include/sparseharness_hip.h, kruskal() the forest that
Kruskal's algorithm returns when it takes the edges in ascending KEY, schedule() a simulator of the round schedule of
csrc/msf.hip.h that returns what the device reports per round, and the makers of the patterns the GPU tests run on."""
import numpy as np

import wcc_ref as W

MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def order_key(bits):
    """k(b) of the header: b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000 (uint32 in, uint32 out)."""
    b = np.asarray(bits, np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def edges(n, rp, ci, va):
    """-> (eu, ev, weight, k): the edges of the simple undirected graph under the entries as the ascending pairs u < v,
    the 32 bits of the chosen entry of each (the smallest by k over both directions and parallel entries) and its k."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    bits = np.ascontiguousarray(va).view(np.uint32)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    ok = (ci >= 0) & (ci < n) & (bits != 0) & (ci != row)
    lo, hi, k = np.minimum(row, ci)[ok], np.maximum(row, ci)[ok], order_key(bits[ok])
    order = np.lexsort((k, hi, lo))
    lo, hi, k = lo[order], hi[order], k[order]
    first = np.ones(len(lo), bool)
    first[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    k = k[first]
    weight = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return lo[first].astype(np.int32), hi[first].astype(np.int32), weight, k


def keys_of(k):
    return (k.astype(np.uint64) << np.uint64(32)) | np.arange(len(k), dtype=np.uint64)


def labels(n, eu, ev, chosen):
    """comp[v] = the largest index of v's component in the forest of the chosen edges (plain union-find)."""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for e in np.nonzero(chosen)[0]:
        a, b = find(int(eu[e])), find(int(ev[e]))
        parent[min(a, b)] = max(a, b)
    return np.array([find(v) for v in range(n)], np.int32)


def kruskal(n, eu, ev, k):
    """-> in_msf (int32, 1 or 0): the edges taken in ascending KEY, each kept when its ends lie in two trees."""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    chosen = np.zeros(len(eu), np.int32)
    for e in np.argsort(keys_of(k), kind="stable"):
        a, b = find(int(eu[e])), find(int(ev[e]))
        if a != b:
            parent[a] = b
            chosen[e] = 1
    return chosen


def schedule(n, rp, ci, va, max_rounds=33):
    """The rounds of msf.hip.h on one state per launch: find (drop the edges inside a tree, the others bid for both
    trees), pick (every root with a bid chooses; of a mutual pair the smaller index hooks), link, jumps until every tree
    is a star.  -> dict(in_msf, comp, weight, eu, ev, M, rounds, complete, walked, kept, hooks, depth, tree_edges,
    components); depth[r]: the deepest vertex behind round r's hooks (what the jump sweeps have to flatten)."""
    eu, ev, weight, k = edges(n, rp, ci, va)
    M = len(eu)
    key = keys_of(k)
    p = np.arange(n, dtype=np.int64)
    lst = np.arange(M, dtype=np.int64)
    in_msf = np.zeros(M, np.int32)
    walked, kept, hooks, depth, complete = [], [], [], [], False
    while n > 0 and len(walked) < max_rounds:
        a, b = p[eu[lst]], p[ev[lst]]
        keep = a != b
        walked.append(len(lst))
        lst, a, b = lst[keep], a[keep], b[keep]
        kept.append(len(lst))
        if len(lst) == 0:
            hooks.append(0)
            depth.append(1 if n else 0)
            complete = True
            break
        best = np.full(n, MAX, np.uint64)
        np.minimum.at(best, a, key[lst])
        np.minimum.at(best, b, key[lst])
        roots = np.nonzero(best != MAX)[0]
        e = (best[roots] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        in_msf[e] = 1
        ra, rb = p[eu[e]], p[ev[e]]
        other = np.where(ra == roots, rb, ra)
        stay = (best[other] == best[roots]) & (roots > other)
        to = np.where(stay, roots, other)
        hooks.append(int((to != roots).sum()))
        p[roots] = to
        d = 1
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p, d = q, 2 * d
        depth.append(d)   # (an upper bound by doubling: the chain is deeper than d / 2)
    if n == 0:
        complete = True
    if complete:
        top = np.zeros(n, np.int64)
        np.maximum.at(top, p, np.arange(n, dtype=np.int64))
        comp = top[p].astype(np.int32)
    else:
        comp = np.full(n, -1, np.int32)
    components = int((p == np.arange(n)).sum())
    return dict(in_msf=in_msf, comp=comp, weight=weight, eu=eu, ev=ev, M=M, rounds=len(walked), complete=complete,
                walked=np.array(walked, np.int64), kept=np.array(kept, np.int64), hooks=np.array(hooks, np.int64),
                depth=depth, tree_edges=n - components, components=components)


# ---- the patterns
def weighted(mat, w, seed=None):
    """The pattern `mat` with new values per stored entry: w is an array, "unit", or "drawn" (float32 in [0, 1) from a
    seeded generator; a drawn 0.0 would be no edge, so it becomes the smallest positive float32)."""
    n, rp, ci, va = mat
    if isinstance(w, str) and w == "unit":
        w = np.ones(len(ci), np.float32)
    elif isinstance(w, str) and w == "drawn":
        w = np.random.default_rng(seed).random(len(ci), dtype=np.float32)
        w[w == 0] = np.float32(1e-45)
    return n, rp, ci, np.ascontiguousarray(w, np.float32)


def by_edge(mat, of_edge):
    """The pattern `mat` where every stored entry of edge e weighs of_edge[e] (float32); entries that are no edges keep
    their values."""
    n, rp, ci, va = mat
    eu, ev, _, _ = edges(n, rp, ci, np.ones(len(ci), np.float32))
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    lo, hi = np.minimum(row, ci), np.maximum(row, ci)
    code = eu.astype(np.int64) * n + ev
    at = np.searchsorted(code, lo * n + hi)
    at = np.minimum(at, max(len(code) - 1, 0))
    out = np.array(va, np.float32)
    hit = (code[at] == lo * n + hi) & (ci != row) if len(code) else np.zeros(len(ci), bool)
    out[hit] = np.asarray(of_edge, np.float32)[at[hit]]
    return n, rp, ci, out


def ruler_path(n=1024):
    """The path 0 - 1 - ... - (n - 1) whose edge i weighs the number of trailing zeros of i + 1, plus 1 (a stored 0.0
    would be no edge; the order of the weights is what counts): the lightest edges pair the vertices up, round after
    round -- log2(n) merging rounds and the empty last one."""
    i = np.arange(1, n, dtype=np.int64)
    tz = np.zeros(n - 1, np.int64)
    for b in range(1, 40):
        tz += (i % (1 << b) == 0)
    return by_edge(W.path(n), (tz + 1).astype(np.float32))


def chain_path(n=70_001, ascending=True):
    """The path of n vertices with strictly ascending (or descending) weights along it: every vertex but one end picks
    the edge towards the light end, so round 1 hooks a single chain of depth n - 1."""
    w = np.arange(1, n, dtype=np.float32)
    return by_edge(W.path(n), w if ascending else w[::-1].copy())


def hub(k=70_001):
    """A hub (vertex 0) with k leaves, drawn weights: one best word wanted by every edge."""
    return weighted(W.csr(k + 1, np.zeros(k, np.int64), np.arange(1, k + 1, dtype=np.int64)), "drawn", seed=3)


def islands():
    """Several components and isolated vertices: three grids of different sizes, a triangle and 11 vertices alone, the
    indices shuffled, drawn weights."""
    src, dst, base = [], [], 0
    for side in (9, 5, 2):
        n, rp, ci, _ = W.grid(side)
        src.append(ci.astype(np.int64) + base)
        dst.append(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) + base)
        base += n
    src.append(np.array([0, 1, 2]) + base)
    dst.append(np.array([1, 2, 0]) + base)
    base += 3 + 11
    name = np.random.default_rng(21).permutation(base)
    return weighted(W.csr(base, name[np.concatenate(src)], name[np.concatenate(dst)]), "drawn", seed=22)


def noise():
    """Only self-loops, stored zeros and columns outside the matrix: no edge."""
    n = 50
    r = np.arange(n, dtype=np.int64)
    rp = (3 * np.arange(n + 1)).astype(np.int32)
    ci = np.stack([r, (r + 1) % n, r + n], axis=1).ravel().astype(np.int32)   # a loop, a stored zero, a column outside
    va = np.stack([np.ones(n), np.zeros(n), np.ones(n)], axis=1).ravel().astype(np.float32)
    return n, rp, ci, va


def graph4(mask, weights):
    """The graph on 4 labelled vertices whose edge (in the order of the pairs u < v) i is present when bit i of mask is
    set, both directions stored; weights: "equal", "ascending" or "descending" in the edge id."""
    pairs = [(u, v) for u in range(4) for v in range(u + 1, 4)]
    have = [pr for i, pr in enumerate(pairs) if mask >> i & 1]
    m = len(have)
    w = {"equal": np.ones(m), "ascending": np.arange(1, m + 1), "descending": np.arange(m, 0, -1)}[weights].astype(np.float32)
    src = np.array([u for u, v in have] + [v for u, v in have], np.int64)
    dst = np.array([v for u, v in have] + [u for u, v in have], np.int64)
    return W.csr(4, src, dst, np.concatenate([w, w]))
