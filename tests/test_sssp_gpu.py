"""sh_sssp on the GPU: distances bit for bit against sh_iterate(SH_MIN_PLUS_F32) run to its exact fixed point and
against the numpy reference written from the definition (tests/sssp_ref.py, itself pinned to the oracle's loop and to
float64 Dijkstra by tests/test_sssp_ref.py); canonical predecessors against the same reference; under the default bucket
width, one bucket (+Inf), the smallest positive weight and one width in between; starts of every kind, the round cap,
reuse of a handle, a graph without rows, the footprint formula, the accounting statement of the header.

Every comparison is exact (== on uint32 / int32 arrays): the fixed point is unique, the predecessors canonical.
"""
import numpy as np
import pytest

import graph_patterns as P
import minplus_ref as M
import sssp_ref as S
from conftest import MATRICES, mtx
from oracle import oracle as O
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

MP = O.MIN_PLUS_F32
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def ragged_square():
    """P.ragged_pattern with real weights of mixed sign, a third of them zero, a few +-Inf."""
    rng, rp, ci = P.ragged_pattern()
    va = M.real_weights(rng, int(rp[-1]))
    va[rng.random(len(va)) < 1.0 / 3.0] = 0.0
    va[rng.choice(len(va), 40, replace=False)] = np.where(rng.random(40) < 0.5, np.inf, -np.inf).astype(np.float32)
    return rp, ci, va


def integer_grid(h=200, w=300, seed=5):
    """4-neighbour grid, vertex (i, j) = i * w + j, integer weights 1..16 (as float32)."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src, dst = [], []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        src += [a.ravel(), b.ravel()]
        dst += [b.ravel(), a.ravel()]
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=h * w))]).astype(np.int32)
    va = np.random.default_rng(seed).integers(1, 17, len(dst)).astype(np.float32)
    return rp, dst.astype(np.int32), va


NAMES = MATRICES + ["ragged", "igrid", "grid", "rmat15", "rmat17"]
FOREST = ("igrid", "grid", "rmat15")   # every weight moves every sum it is added to (asserted below): pred is a forest
_cache, _refs = {}, {}


def matrix(name):
    """(n, row_ptr, col_idx, float32 values) of a test matrix."""
    if name not in _cache:
        if name == "ragged":
            rp, ci, va = ragged_square()
        elif name == "igrid":
            rp, ci, va = integer_grid()
        elif name in M.GRAPHS:
            rp, ci, va, _ = M.graph(name)
        elif name == "rmat17":   # long rows and long out-lists
            rp, ci, _ = H.rmat(17, seed=40)
            va = M.real_weights(np.random.default_rng(41), len(ci))
        elif name == "edges":    # list lengths on the kernels' thresholds
            rp, ci = P.edges_pattern()
            va = M.real_weights(np.random.default_rng(78), len(ci))
        else:
            rows, cols, _, rp, ci, va = H.mm_load(mtx(name))
            assert rows == cols
        _cache[name] = (len(rp) - 1, rp, ci, np.ascontiguousarray(va, np.float32))
    return _cache[name]


def reference(name, x0, mat=None):
    key = (name, x0.tobytes())
    if key not in _refs:
        n, rp, ci, va = matrix(name) if mat is None else mat
        _refs[key] = S.sssp(rp, ci, va, x0)
    return _refs[key]


def widths(name):
    """default, one bucket, the smallest positive weight, one in between (the geometric mean of that and the largest)."""
    n, rp, ci, va = matrix(name)
    _, _, w = S.edges_of(n, rp, ci, va)
    pos = w[w > 0]
    if len(pos) == 0:
        return (-1.0, INF, 1.0, 2.0)
    return (-1.0, INF, float(pos.min()), float(np.sqrt(float(pos.min()) * float(pos.max())) * 1.5))


def run(eng, G, x0, delta=-1.0, with_pred=True, cap=1 << 20):
    n = len(x0)
    x0 = np.ascontiguousarray(x0, np.float32)
    xv, dv = eng.vector(x0), eng.alloc(max(n, 1)).fill(7.0)
    pv = eng.alloc(max(n, 1)).fill(7, np.int32) if with_pred else None
    res = eng.sssp(G, xv, dv, pv, delta=delta, max_rounds=cap)
    dist = dv.download(np.float32, n=n)
    pred = pv.download(np.int32, n=n) if with_pred else None
    np.testing.assert_array_equal(xv.download(np.uint32, n=n), M.bits(x0))   # x0 is only read
    for v in (xv, dv, pv):
        if v is not None:
            v.free()
    return dist, pred, res


def check(name, x0, dist, pred, res, what="", mat=None):
    want_dist, want_pred, want_reached, outdeg_sum = reference(name, x0, mat)
    rounds, buckets, reached, complete, relaxed, sizes, edges, per, total = res
    print(f"{name} {what}: rounds {rounds} buckets {buckets} reached {reached} relaxed {relaxed} (out-degrees of the reached: "
          f"{outdeg_sum}) total_ns {total}")
    np.testing.assert_array_equal(M.bits(dist), M.bits(want_dist), err_msg=f"{name} {what} dist")
    if pred is not None:
        np.testing.assert_array_equal(pred, want_pred, err_msg=f"{name} {what} pred")
    assert complete and reached == want_reached, (name, what)
    assert relaxed >= outdeg_sum, (name, what)
    assert len(sizes) == len(edges) == len(per) == rounds and int(edges.sum()) == relaxed
    assert total >= int(np.sum(per))


def iterate_arm(eng, name, x0):
    """sh_iterate(SH_MIN_PLUS_F32, 0, 0, y0 = x0) on the matrix under its default plan, to its exact fixed point."""
    n, rp, ci, va = matrix(name)
    A = eng.upload_csr(n, n, rp, ci, va)
    xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0.0)
    iters, conv, _, _ = eng.iterate(MP, A, xv, yv, sc, 0.0, 0.0, delta=1e-30, max_iters=n + 1)
    out = xv.download(np.float32)
    assert conv
    for v in (xv, yv, sc, A):
        v.free()
    return out, iters


# ------------------------------------------------------------------ 1. every matrix, every bucket width
@pytest.mark.parametrize("name", NAMES + ["edges"])
def test_dist_and_pred_under_every_bucket_width(eng, name):
    n, rp, ci, va = matrix(name)
    if name == "edges":
        P.assert_edge_lengths(rp, ci)
    G = eng.sssp_graph(rp, ci, va)
    for source in P.sources(name):
        dist_and_pred_under_every_bucket_width(eng, name, G, source)
    G.free()


def dist_and_pred_under_every_bucket_width(eng, name, G, source):
    n, rp, ci, va = matrix(name)
    x0 = M.start_vector(n, source)
    want_dist, want_pred, _, _ = reference(name, x0)
    it_dist, iters = iterate_arm(eng, name, x0)
    np.testing.assert_array_equal(M.bits(it_dist), M.bits(want_dist), err_msg=f"{name}: sh_iterate against the reference")
    c, r, w = S.edges_of(n, rp, ci, va)
    assert G.edges == len(c)
    for delta in widths(name):
        dist, pred, res = run(eng, G, x0, delta)
        np.testing.assert_array_equal(M.bits(dist), M.bits(it_dist), err_msg=f"{name} delta {delta}: against sh_iterate")
        check(name, x0, dist, pred, res, f"delta {delta}")
    dist, _, res = run(eng, G, x0, with_pred=False)   # without the predecessor pass
    check(name, x0, dist, None, res, "no pred")
    if name in FOREST:
        assert (want_dist[c] + w > want_dist[c])[want_dist[c] < M.FLT_MAX].all()
        dist, pred, _ = run(eng, G, x0)
        assert S.walk_to_roots(dist, pred) >= 3
        assert (pred[dist < M.FLT_MAX] >= 0).sum() == int((dist < M.FLT_MAX).sum()) - 1
    if name == "ragged":
        assert np.bincount(r, minlength=n).max() > 4096 and np.bincount(c, minlength=n).max() > 2048   # pieces in both kernels
        assert (w == 0).mean() > 0.25 and np.isinf(va).sum() == 40 and (va < 0).any() and ((ci < 0) | (ci >= n)).any()
    if name == "igrid":
        assert iters > 300
    if name == "rmat17":
        assert np.bincount(c, minlength=n).max() > 2048


# ------------------------------------------------------------------ 2. starts of every kind
@pytest.mark.parametrize("name", ["matrix", "matrix2", "ragged", "igrid", "rmat15"])
def test_starts(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.sssp_graph(rp, ci, va)
    c, _, _ = S.edges_of(n, rp, ci, va)
    outdeg = np.bincount(c, minlength=n)
    rng = np.random.default_rng(11)
    three = np.full(n, M.FLT_MAX, np.float32)
    three[rng.choice(n, 3, replace=False)] = [0.0, 3.25, 40.0]          # three sources with offsets
    signed = three.copy()
    signed[signed < M.FLT_MAX] *= -1.0                                  # the sign of x0 does not matter ...
    signed[::3] *= -1.0                                                 # ... nor does that of FLT_MAX
    cases = {"three": three, "signed": signed, "none": np.full(n, M.FLT_MAX, np.float32)}
    leaves = np.flatnonzero(outdeg == 0)
    if len(leaves):
        cases["leaf"] = M.start_vector(n, int(leaves[0]))
    for what, x0 in cases.items():
        for delta in (-1.0, INF, widths(name)[3]):
            dist, pred, res = run(eng, G, x0, delta)
            check(name, x0, dist, pred, res, f"{what} delta {delta}")
        if what == "signed":
            np.testing.assert_array_equal(M.bits(dist), M.bits(reference(name, three)[0]))
        if what == "none":
            assert res[0] == 0 and res[2] == 0 and res[3] and (M.bits(dist) == S.FLT_MAX_BITS).all() and (pred == -1).all()
        if what == "leaf":
            assert res[2] == 1 and res[4] == 0 and (pred == -1).all()
    if name == "rmat15":   # (an R-MAT has vertices no row reads)
        assert "leaf" in cases
    G.free()


# ------------------------------------------------------------------ 3. the round cap, and reuse of the handle
def test_one_round_leaves_a_vector_between_the_fixed_point_and_the_start(eng):
    name = "igrid"
    n, rp, ci, va = matrix(name)
    x0 = M.start_vector(n, 0)
    want_dist, _, _, _ = reference(name, x0)
    G = eng.sssp_graph(rp, ci, va)
    xv, dv, pv = eng.vector(x0), eng.alloc(n).fill(7.0), eng.alloc(n).fill(7, np.int32)
    rounds, buckets, reached, complete, relaxed, sizes, edges, per, total = eng.sssp(G, xv, dv, pv, max_rounds=1)
    dist = dv.download(np.float32)
    assert (rounds, complete) == (1, False) and 1 < reached < n
    assert (M.bits(want_dist) <= M.bits(dist)).all() and (M.bits(dist) <= M.bits(S.start(x0))).all()
    assert (pv.download(np.int32) == 7).all()                           # pred is not written by a cut search
    for v in (xv, dv, pv):
        v.free()
    # the same handle then gives the full result, from here and from elsewhere
    for source in (0, n - 1, n // 2 + 17):
        x0 = M.start_vector(n, source)
        for delta in (-1.0, 7.0):
            dist, pred, res = run(eng, G, x0, delta)
            check(name, x0, dist, pred, res, f"after a cut call, source {source} delta {delta}")
    G.free()


# ------------------------------------------------------------------ 4. handle queries
def footprint_formula(rows, edges):
    return 8 * (rows + 1) + 16 * edges + 20 * rows + 16 * (edges // 1024 + 1) + 8 * (edges // 2048 + 1) + 22528


@pytest.mark.parametrize("name", NAMES)
def test_footprint_edges_and_default_width(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.sssp_graph(rp, ci, va)
    c, r, w = S.edges_of(n, rp, ci, va)
    assert G.edges == len(c)
    assert G.footprint == footprint_formula(n, len(c))
    assert len(c) > 0 and 0 < G.delta < INF
    if w.sum() > 0:   # the header's formula: 32 * (sum of the weights / edges) * (rows / edges)
        assert G.delta == pytest.approx(32.0 * (float(w.astype(np.float64).sum()) / len(c)) * (n / len(c)), rel=1e-9)
    if name == "ragged":
        assert len(c) < len(ci) - 1000   # the edge filter is really exercised
    G.free()


def test_a_graph_without_rows_and_one_without_entries(eng):
    G = eng.sssp_graph(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert G.edges == 0 and G.footprint == footprint_formula(0, 0) and G.delta == 0.0
    xv, dv = eng.alloc(1), eng.alloc(1)
    rounds, buckets, reached, complete, relaxed, sizes, edges, per, total = eng.sssp(G, xv, dv, None, max_rounds=10)
    assert (rounds, buckets, reached, complete, relaxed, len(sizes), total) == (0, 0, 0, True, 0, 0, 0)
    for h in (xv, dv, G):
        h.free()
    n = 100
    G = eng.sssp_graph(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert G.delta == 0.0 and G.footprint == footprint_formula(n, 0)
    x0 = np.full(n, M.FLT_MAX, np.float32)
    x0[[3, 4]] = [0.0, 1.5]
    for delta in (-1.0, INF, 0.5):
        dist, pred, res = run(eng, G, x0, delta)
        np.testing.assert_array_equal(M.bits(dist), M.bits(x0))
        assert (pred == -1).all() and res[2] == 2 and res[3] and res[4] == 0
    G.free()


def test_stored_zeros_are_edges_and_infinite_weights_are_not(eng):
    rp = np.array([0, 0, 1, 2, 3, 4], np.int32)                   # 0 -> 1 (0.0), 1 -> 2 (-0.0), 2 -> 3 (inf), 3 -> 4 (1.0)
    ci = np.array([0, 1, 2, 3], np.int32)
    va = np.array([0.0, -0.0, np.inf, 1.0], np.float32)
    G = eng.sssp_graph(rp, ci, va)
    assert G.edges == 3 and G.delta > 0
    for delta in (-1.0, INF, 0.25):
        dist, pred, res = run(eng, G, M.start_vector(5, 0), delta)
        assert M.bits(dist).tolist() == [0, 0, 0, S.FLT_MAX_BITS, S.FLT_MAX_BITS]
        assert pred.tolist() == [-1, 0, 1, -1, -1] and res[2] == 3 and res[3] and res[4] >= 2
    G.free()


def test_errors(eng):
    n, rp, ci, va = matrix("matrix3")
    G = eng.sssp_graph(rp, ci, va)
    xv, dv, pv, short = eng.alloc(n).fill(0.0), eng.alloc(n), eng.alloc(n), eng.alloc(n - 1)
    with pytest.raises(EngineError, match="alias"):
        eng.sssp(G, xv, xv, None, max_rounds=10)
    with pytest.raises(EngineError, match="alias"):
        eng.sssp(G, xv, dv, dv, max_rounds=10)
    with pytest.raises(EngineError, match="alias"):
        eng.sssp(G, xv, dv, xv, max_rounds=10)
    with pytest.raises(EngineError, match="dist is shorter"):
        eng.sssp(G, xv, short, None, max_rounds=10)
    with pytest.raises(EngineError, match="pred is shorter"):
        eng.sssp(G, xv, dv, short, max_rounds=10)
    with pytest.raises(EngineError, match="x0 is shorter"):
        eng.sssp(G, short, dv, None, max_rounds=10)
    with pytest.raises(EngineError, match="max_rounds"):
        eng.sssp(G, xv, dv, pv, max_rounds=0)
    with pytest.raises(EngineError, match="NaN"):
        eng.sssp(G, xv, dv, pv, delta=float("nan"), max_rounds=10)
    bad = rp.copy()
    bad[-1] += 1
    with pytest.raises(EngineError, match="row_ptr"):
        eng.sssp_graph(bad, ci, va)
    for h in (G, xv, dv, pv, short):
        h.free()
