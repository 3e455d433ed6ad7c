"""The numpy reference of sh_sssp, written from the definition in include/sparseharness_hip.h, and the inputs that
tests/test_sssp_ref.py checks on the CPU and tests/test_sssp_gpu.py compares the engine with.  Not a test, not a conftest.

dist: iterate minplus_ref.order_free (one (min,+) launch without any order) with alpha = beta = 0 and y = x until no bit
changes.  That is the greatest F <= d0 with F[r] <= fl32(F[c] + w) on every edge: each launch computes
F_(k+1)[r] = min(F_k[r], min_c fl32(F_k[c] + w)), fl32 is monotone, so F_k never goes below the greatest such vector and
stops exactly on it.  pred: the rule, in three numpy lines.
"""
import numpy as np

import minplus_ref as M

FLT_MAX = M.FLT_MAX
FLT_MAX_BITS = 0x7F7FFFFF


def edges_of(n, rp, ci, va):
    """(c, r, w) of every edge c -> r: row r stores column c, 0 <= c < n, with a value of finite magnitude; w = |a|."""
    ci = np.asarray(ci, np.int64)
    w = np.abs(np.ascontiguousarray(va).view(np.float32))
    keep = (ci >= 0) & (ci < n) & np.isfinite(w)
    return ci[keep], M.rows_of_entries(rp)[keep], w[keep]


def start(x0):
    """d0 = |x0|, an infinite start counted as FLT_MAX."""
    return np.minimum(np.abs(np.ascontiguousarray(x0, np.float32)), FLT_MAX)


def fixed_point(rp, ci, va, x0, max_launches=100_000):
    """-> (dist, launches that changed something)."""
    n = len(rp) - 1
    va = np.ascontiguousarray(va).view(np.float32)
    x = start(x0)
    for k in range(max_launches):
        nxt = M.order_free(rp, ci, va, x, x, 0.0, 0.0, n)
        if np.array_equal(M.bits(nxt), M.bits(x)):
            return x, k
        x = nxt
    raise AssertionError("no fixed point")


def predecessors(n, rp, ci, va, x0, dist, without_bit_test=False):
    """pred[v] = -1 where bits(dist[v]) == bits(d0[v]), else the smallest c with an edge c -> v and
    bits(fl32(dist[c] + w)) == bits(dist[v]).  `without_bit_test` is the mutant that takes the smallest c of any edge."""
    c, r, w = edges_of(n, rp, ci, va)
    moved = M.bits(dist) != M.bits(start(x0))
    with np.errstate(over="ignore"):
        through = dist[c] + w                      # float32 + float32: one rounding
    assert through.dtype == np.float32
    ok = moved[r] & (True if without_bit_test else M.bits(through) == M.bits(dist)[r])
    pred = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(pred, r[ok], c[ok])
    pred[pred == np.iinfo(np.int64).max] = -1
    return pred.astype(np.int32), moved


def sssp(rp, ci, va, x0):
    """-> (dist, pred, reached, sum of the out-degrees of the reached vertices)"""
    n = len(rp) - 1
    dist, _ = fixed_point(rp, ci, va, x0)
    pred, moved = predecessors(n, rp, ci, va, x0, dist)
    assert ((pred >= 0) == moved).all(), "at a fixed point every moved vertex has a predecessor"
    c, _, _ = edges_of(n, rp, ci, va)
    outdeg = np.bincount(c, minlength=n)
    reached = dist < FLT_MAX
    return dist, pred, int(reached.sum()), int(outdeg[reached].sum())


def float64_mutant(rp, ci, va, x0, max_launches=100_000):
    """The mutant that adds in float64 and rounds the vector once per launch."""
    n = len(rp) - 1
    c, r, w = edges_of(n, rp, ci, va)
    x = start(x0).astype(np.float64)
    for _ in range(max_launches):
        nxt = x.copy()
        np.minimum.at(nxt, r, x[c] + w.astype(np.float64))
        nxt = np.minimum(nxt, float(FLT_MAX))
        if np.array_equal(nxt, x):
            return x.astype(np.float32)
        x = nxt
    raise AssertionError("no fixed point")


def push_bellman_ford(rp, ci, va, x0, rng, delta):
    """A push-order, bucketed label-correcting search: the edges in a random order, cut into random chunks that are
    relaxed one after the other on the vector of the moment; only vertices below the threshold push, and the threshold
    moves up by buckets of `delta` when a whole pass improved nothing.  -> dist"""
    n = len(rp) - 1
    c, r, w = edges_of(n, rp, ci, va)
    perm = rng.permutation(len(c))
    c, r, w = c[perm], r[perm], w[perm]
    cuts = np.sort(rng.integers(0, len(c) + 1, 7))
    chunks = [s for s in np.split(np.arange(len(c)), cuts) if len(s)]
    dist = start(x0).copy()
    thr = float(delta)
    while True:
        improved = False
        for s in chunks:
            src = dist[c[s]]
            act = src.astype(np.float64) < thr
            with np.errstate(over="ignore"):
                nd = src[act] + w[s][act]
            tgt = r[s][act]
            old = dist[tgt]
            np.minimum.at(dist, tgt, nd)
            improved = improved or bool((dist[tgt] < old).any())
        if improved:
            continue
        waiting = dist[(dist < FLT_MAX) & (dist.astype(np.float64) >= thr)]
        if len(waiting) == 0:
            return dist
        thr = (np.floor(float(waiting.min()) / delta) + 1.0) * delta if np.isfinite(delta) else np.inf
        if not thr > float(waiting.min()):
            thr = np.inf


def walk_to_roots(dist, pred):
    """From every vertex with a predecessor up its chain: dist must fall strictly at every step and the chain must end
    at a vertex without one.  -> the longest chain"""
    at = np.nonzero(pred >= 0)[0]
    steps = 0
    while len(at):
        up = pred[at].astype(np.int64)
        assert (dist[up] < dist[at]).all(), "dist does not grow strictly along pred"
        at = up[pred[up] >= 0]
        steps += 1
        assert steps <= len(dist), "a cycle in pred"
    return steps
