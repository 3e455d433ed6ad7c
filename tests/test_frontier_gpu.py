"""sh_iterate_frontier on the GPU: the transposed pattern, equality with sh_iterate and the oracle bit for bit (final
vector, launch count, converged flag), the bookkeeping (changed / active rows per launch) against the algorithm's own
definition computed in numpy, inputs that are not monotone, reuse of a handle, the launch cap."""
import numpy as np
import pytest

import graph_patterns as P
import minplus_ref as M
from conftest import MATRICES, mtx
from oracle import oracle as O
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine

pytestmark = pytest.mark.gpu

SEMIRINGS = [O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32]
SHARES = [0.0, 1.0, -1.0]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


rows_of_entries = P.rows_of_entries


def scc_values(rp, ci):
    """scc_normalise on a CSR: the row index off the diagonal, INT_MIN on it (src/sparse_matrix.cpp:433-456)."""
    r = rows_of_entries(rp)
    return np.where(ci == r, np.int32(O.INT_MIN), r).astype(np.int32)


def ragged_square():
    """P.ragged_pattern with small integer values, a third of them stored zeros."""
    rng, rp, ci = P.ragged_pattern()
    va = rng.integers(0, 3, rp[-1]).astype(np.int32)   # a third of the stored values are 0
    return rp, ci, va


def grid_graph(h=200, w=300, seed=5):
    """4-neighbour grid, vertex (i, j) = i * w + j, integer weights 1..16."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src, dst = [], []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        src += [a.ravel(), b.ravel()]
        dst += [b.ravel(), a.ravel()]
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=h * w))]).astype(np.int32)
    va = np.random.default_rng(seed).integers(1, 17, len(dst)).astype(np.int32)
    return rp, dst.astype(np.int32), va


_cache = {}


def matrix(name):
    """(n, row_ptr, col_idx, integer values) of a test matrix."""
    if name not in _cache:
        if name == "ragged":
            rp, ci, va = ragged_square()
        elif name == "grid":
            rp, ci, va = grid_graph()
        elif name == "edges":   # list lengths on the kernels' thresholds; ones (real weights for (min,+): see case)
            rp, ci = P.edges_pattern()
            va = np.ones(len(ci), np.int32)
        else:
            rows, cols, _, rp, ci, va = H.mm_load(mtx(name), elem_is_int=True)
            assert rows == cols
        _cache[name] = (len(rp) - 1, rp, ci, va)
    return _cache[name]


def case(sr, name, source=0):
    """(n, rp, ci, values, x0, y0, alpha, beta) of the app that runs `sr`, on matrix `name`, started from `source`."""
    n, rp, ci, va = matrix(name)
    x0 = O.initial_vector(sr, n)
    if sr != O.MAX_MIN_I32:     # (the SCC labels have no source)
        x0 = np.roll(x0, source)
    if sr == O.MIN_PLUS_F32:    # SSSP (app/sssp.cpp)
        vals = M.real_weights(np.random.default_rng(78), len(ci)) if name == "edges" else va.astype(np.float32)
        return n, rp, ci, vals, x0, x0, 0.0, 0.0
    if sr == O.OR_AND_I32:      # BFS that keeps what it has reached
        return n, rp, ci, va, x0, x0, 1, 1
    return n, rp, ci, scc_values(rp, ci), x0, np.full(n, O.INT_MIN, np.int32), O.INT_MAX, O.INT_MIN   # SCC labels (app/scc.cpp)


def run_frontier(eng, sr, A, F, x0, y0, a, b, share, delta=1e-4, cap=2000):
    dt = O.elem_dtype(sr)
    xv, yv, sc = eng.vector(x0.astype(dt)), eng.vector(y0.astype(dt)), eng.alloc(len(x0)).fill(0)
    res = eng.iterate_frontier(sr, A, F, xv, yv, sc, a, b, delta=delta, max_iters=cap, dense_share=share)
    got = xv.download(dt)
    for v in (xv, yv, sc):
        v.free()
    return got, res


def run_dense(eng, sr, A, x0, y0, a, b, delta=1e-4, cap=2000):
    dt = O.elem_dtype(sr)
    xv, yv, sc = eng.vector(x0.astype(dt)), eng.vector(y0.astype(dt)), eng.alloc(len(x0)).fill(0)
    iters, conv, _, _ = eng.iterate(sr, A, xv, yv, sc, a, b, delta=delta, max_iters=cap)
    got = xv.download(dt)
    for v in (xv, yv, sc):
        v.free()
    return got, iters, conv


# ------------------------------------------------------------------ 1. the transposed pattern
@pytest.mark.parametrize("name", MATRICES + ["ragged", "edges"])
@pytest.mark.parametrize("plan", [1, 2])
def test_transpose(eng, name, plan):
    n, rp, ci, va = matrix(name)
    A = eng.upload_csr(n, n, rp, ci, va, plan=plan)
    F = eng.frontier(A, rp, ci, va)
    col_ptr, row_of = F.transpose()
    inb = (ci >= 0) & (ci < n)
    cols, rows = ci[inb], rows_of_entries(rp)[inb]
    order = np.argsort(cols, kind="stable")
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    np.testing.assert_array_equal(col_ptr, want_ptr)
    got = row_of.copy()
    for c in range(n):   # the order inside a column is unspecified
        got[col_ptr[c]:col_ptr[c + 1]].sort()
    np.testing.assert_array_equal(got, rows[order])   # (rows ascend inside a column of a stable sort of the CSR walk)
    if name == "ragged":
        assert np.diff(col_ptr).max() == 20_001 and np.diff(rp).max() >= 20_001
    if name == "edges":
        P.assert_edge_lengths(rp, ci)
    F.free()
    A.free()


# ------------------------------------------------------------------ 2. equality with sh_iterate and the oracle
def uploads(sr):
    ups = [dict(plan=1), dict(plan=2)]
    if sr == O.OR_AND_I32:
        ups.append(dict(or_and_bits=2))
    return ups


@pytest.mark.parametrize("name", MATRICES + ["ragged", "grid", "edges"])
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_equals_iterate_and_oracle(eng, sr, name):
    if name == "edges":
        P.assert_edge_lengths(*matrix(name)[1:3])
    for source in P.sources(name) if sr != O.MAX_MIN_I32 else (0,):
        equals_iterate_and_oracle(eng, sr, name, source)


def equals_iterate_and_oracle(eng, sr, name, source):
    n, rp, ci, vals, x0, y0, a, b = case(sr, name, source)
    want, w_it, w_conv = O.iterate(sr, rp, ci, vals, x0, y0, a, b, 1e-4, 2000)
    if name == "grid" and sr != O.MAX_MIN_I32:   # (the SCC labels of a grid settle in two launches)
        assert w_conv and w_it > 400   # the wavefront crosses 498 edges
    for up in uploads(sr):
        A = eng.upload_csr(n, n, rp, ci, vals, **up)
        F = eng.frontier(A, rp, ci, vals)
        d_got, d_it, d_conv = run_dense(eng, sr, A, x0, y0, a, b)
        assert (d_it, d_conv) == (w_it, w_conv)
        np.testing.assert_array_equal(bits(d_got), bits(want))
        for share in SHARES:
            got, (it, conv, modes, changed, active, per, total) = run_frontier(eng, sr, A, F, x0, y0, a, b, share)
            assert (it, conv) == (w_it, w_conv), f"{up} dense_share {share} source {source}: {it} launches, converged {conv}"
            np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{up} dense_share {share} source {source}")
            assert len(modes) == len(per) == it and total == sum(per)
            if share == 0.0:
                assert not any(modes) and all(k == n for k in active)
            if share == 1.0:
                assert modes == [0, 0][:it] + [1] * max(it - 2, 0)
        F.free()
        A.free()


@pytest.mark.parametrize("sr", [O.MIN_PLUS_F32, O.OR_AND_I32])
def test_the_apps_own_scalars_on_reference_matrices(eng, sr, matrix_name):
    """BFS as the app launches it (alpha = 1, beta = 0: a vertex does not keep its mark) and SSSP."""
    n, rp, ci, vals, x0, y0, _, _ = case(sr, matrix_name)
    a, b = (0.0, 0.0) if sr == O.MIN_PLUS_F32 else (1, 0)
    want, w_it, w_conv = O.iterate(sr, rp, ci, vals, x0, y0, a, b, 1e-4, 300)
    A = eng.upload_csr(n, n, rp, ci, vals)
    F = eng.frontier(A, rp, ci, vals)
    for share in SHARES:
        got, res = run_frontier(eng, sr, A, F, x0, y0, a, b, share, cap=300)
        assert res[:2] == (w_it, w_conv)
        np.testing.assert_array_equal(bits(got), bits(want))
    F.free()
    A.free()


# ------------------------------------------------------------------ 3. the bookkeeping is the algorithm's
def oracle_iterates(sr, rp, ci, vals, x0, y0, a, b, launches):
    xs, y = [np.asarray(x0, O.elem_dtype(sr))], y0
    for _ in range(launches):
        xs.append(O.kernel(sr, rp, ci, vals, xs[-1], y, a, b))
        y = xs[-1]
    return xs


def active_rows(rp, ci, n, cmask):
    """|C u rows that hold an entry of a column in C|"""
    inb = (ci >= 0) & (ci < n)
    hit = np.zeros(len(ci), bool)
    hit[inb] = cmask[ci[inb]]
    act = cmask.copy()
    act[rows_of_entries(rp)[hit]] = True
    return int(act.sum())


@pytest.mark.parametrize("name", ["matrix", "matrix3", "ragged", "grid"])
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_changed_and_active_rows_per_launch(eng, sr, name):
    n, rp, ci, vals, x0, y0, a, b = case(sr, name)
    A = eng.upload_csr(n, n, rp, ci, vals)
    F = eng.frontier(A, rp, ci, vals)
    got, (it, conv, modes, changed, active, _, _) = run_frontier(eng, sr, A, F, x0, y0, a, b, 1.0)
    xs = oracle_iterates(sr, rp, ci, vals, x0, y0, a, b, it)
    np.testing.assert_array_equal(bits(got), bits(xs[it]))
    diff = [bits(xs[k + 1]) != bits(xs[k]) for k in range(it)]
    assert changed == [int(d.sum()) for d in diff]
    assert modes == [0, 0][:it] + [1] * max(it - 2, 0)
    assert active[:2] == [n, n][:it]
    assert active[2:] == [active_rows(rp, ci, n, diff[k - 1]) for k in range(2, it)]
    for share in (0.0, -1.0):   # the changed rows do not depend on who computed them
        _, res = run_frontier(eng, sr, A, F, x0, y0, a, b, share)
        assert res[3] == changed
    if name == "grid" and sr == O.OR_AND_I32:
        # derived, not measured: the BFS wavefront from a corner of a 200 x 300 grid is an anti-diagonal of at most 200
        # vertices, so with their neighbours at most 1 000 of the 60 000 rows are active per launch
        assert sum(active) < it * n / 10
        assert max(active[2:]) <= 1000
    F.free()
    A.free()


# ------------------------------------------------------------------ 4. inputs that are not monotone
def cycle_and_path(n=40):
    """A directed 2-cycle 0 <-> 1 and a path 1 -> 2 -> ... -> n-1 hanging off it (row r holds the vertices it reads)."""
    rows = [[1], [0]] + [[r - 1] for r in range(2, n)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return n, rp, ci, np.ones(len(ci), np.int32)


@pytest.mark.parametrize("cap", [37, 38])
@pytest.mark.parametrize("share", SHARES)
def test_oscillating_bfs_never_converges(eng, cap, share):
    """alpha = 1, beta = 0: the mark runs round the 2-cycle for ever and every other launch sends one down the path.
    A loop that stops when the changed list is empty, or that reads a stale ping-pong buffer, differs here."""
    n, rp, ci, va = cycle_and_path()
    x0 = O.initial_vector(O.OR_AND_I32, n)
    want, w_it, w_conv = O.iterate(O.OR_AND_I32, rp, ci, va, x0, x0, 1, 0, 1e-4, cap)
    assert (w_it, w_conv) == (cap, False)
    A = eng.upload_csr(n, n, rp, ci, va)
    F = eng.frontier(A, rp, ci, va)
    got, res = run_frontier(eng, O.OR_AND_I32, A, F, x0, x0, 1, 0, share, cap=cap)
    assert res[:2] == (cap, False)
    np.testing.assert_array_equal(got, want)
    F.free()
    A.free()


@pytest.mark.parametrize("share", SHARES)
def test_min_plus_with_growing_values_and_coarse_deltas(eng, share):
    n, rp, ci, va = matrix("grid")
    vals = va.astype(np.float32)
    x0 = O.initial_vector(O.MIN_PLUS_F32, n)
    A = eng.upload_csr(n, n, rp, ci, vals)
    F = eng.frontier(A, rp, ci, vals)
    # beta = 0.5: every launch adds to every reached value; capped
    want, w_it, w_conv = O.iterate(O.MIN_PLUS_F32, rp, ci, vals, x0, x0, 0.0, 0.5, 1e-4, 25)
    got, res = run_frontier(eng, O.MIN_PLUS_F32, A, F, x0, x0, 0.0, 0.5, share, cap=25)
    assert res[:2] == (w_it, w_conv)
    np.testing.assert_array_equal(bits(got), bits(want))
    # delta = 2.5: improvements of 1 or 2 change bits but do not count as differing -- the loop stops where sh_iterate
    # stops, with the changed list still non-empty
    want, w_it, w_conv = O.iterate(O.MIN_PLUS_F32, rp, ci, vals, x0, x0, 0.0, 0.0, 2.5, 2000)
    full, f_it, _ = O.iterate(O.MIN_PLUS_F32, rp, ci, vals, x0, x0, 0.0, 0.0, 1e-4, 2000)
    got, res = run_frontier(eng, O.MIN_PLUS_F32, A, F, x0, x0, 0.0, 0.0, share, delta=2.5)
    assert res[:2] == (w_it, w_conv)
    np.testing.assert_array_equal(bits(got), bits(want))
    if w_it < f_it:
        assert res[3][-1] > 0   # (the confirming launch still changed bits)
    d_got, d_it, d_conv = run_dense(eng, O.MIN_PLUS_F32, A, x0, x0, 0.0, 0.0, delta=2.5)
    assert (d_it, d_conv) == (w_it, w_conv)
    np.testing.assert_array_equal(bits(d_got), bits(want))
    # delta above FLT_MAX: nothing ever differs
    want, w_it, w_conv = O.iterate(O.MIN_PLUS_F32, rp, ci, vals, x0, x0, 0.0, 0.0, 1e39, 2000)
    got, res = run_frontier(eng, O.MIN_PLUS_F32, A, F, x0, x0, 0.0, 0.0, share, delta=1e39)
    assert res[:2] == (w_it, w_conv) == (1, True)
    np.testing.assert_array_equal(bits(got), bits(want))
    F.free()
    A.free()


# ------------------------------------------------------------------ 5. reuse, footprint
def footprint_formula(n, nnz, copied):
    return (4 * (n + 1) + 8 * nnz if copied else 0) + 4 * (n + 1) + 4 * nnz + 16 * n + 8 * (nnz // 1024 + 1) + 8 * (nnz // 2048 + 1) + 512


@pytest.mark.parametrize("sr", [O.MIN_PLUS_F32, O.OR_AND_I32])
def test_a_handle_serves_many_runs(eng, sr):
    n, rp, ci, vals, x0, y0, a, b = case(sr, "grid")
    A = eng.upload_csr(n, n, rp, ci, vals)
    F = eng.frontier(A, rp, ci, vals)
    for source in (0, n - 1, n // 2 + 17, 0):
        xs = np.roll(x0, source)   # the start vector of another source
        want, w_it, w_conv = O.iterate(sr, rp, ci, vals, xs, xs, a, b, 1e-4, 2000)
        fresh = eng.frontier(A, rp, ci, vals)
        for handle in (F, fresh):
            got, res = run_frontier(eng, sr, A, handle, xs, xs, a, b, 1.0)
            assert res[:2] == (w_it, w_conv)
            np.testing.assert_array_equal(bits(got), bits(want))
        fresh.free()
    F.free()
    A.free()


@pytest.mark.parametrize("name", ["matrix2", "ragged", "grid"])
def test_footprint_is_the_documented_formula(eng, name):
    n, rp, ci, va = matrix(name)
    for up in (dict(plan=1), dict(plan=2), dict(or_and_bits=2)):
        A = eng.upload_csr(n, n, rp, ci, va, **up)
        F = eng.frontier(A, rp, ci, va)
        copied = A.plan()[0] != "stream"   # a matrix that keeps its CSR arrays lends them
        assert copied == (up != dict(plan=1)) or name != "grid"
        assert F.footprint() == footprint_formula(n, int(rp[-1]), copied)
        F.free()
        A.free()


# ------------------------------------------------------------------ 6. the launch cap
@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_cap(eng, sr, cap):
    n, rp, ci, vals, x0, y0, a, b = case(sr, "ragged" if sr == O.MAX_MIN_I32 else "grid")   # (none converges in 3 launches)
    xs = oracle_iterates(sr, rp, ci, vals, x0, y0, a, b, cap)
    assert O.iterate(sr, rp, ci, vals, x0, y0, a, b, 1e-4, cap)[1:] == (cap, False)
    A = eng.upload_csr(n, n, rp, ci, vals)
    F = eng.frontier(A, rp, ci, vals)
    for share in SHARES:
        got, res = run_frontier(eng, sr, A, F, x0, y0, a, b, share, cap=cap)
        assert res[:2] == (cap, False)
        np.testing.assert_array_equal(bits(got), bits(xs[cap]))
    F.free()
    A.free()


def test_errors(eng):
    from sparseharness_amd.engine import EngineError
    n, rp, ci, va = matrix("matrix2")
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    n2, rp2, ci2, va2 = matrix("matrix3")
    B = eng.upload_csr(n2, n2, rp2, ci2, va2, plan=1)
    F = eng.frontier(A, rp, ci, va)
    xv, sc = eng.alloc(max(n, n2)).fill(0), eng.alloc(max(n, n2)).fill(0)
    with pytest.raises(EngineError, match="another matrix"):
        eng.iterate_frontier(O.OR_AND_I32, B, F, xv, xv, sc, 1, 1)
    with pytest.raises(EngineError, match="alias"):
        eng.iterate_frontier(O.OR_AND_I32, A, F, xv, xv, xv, 1, 1)
    with pytest.raises(EngineError, match="SH_PLUS_TIMES_F32"):
        eng.iterate_frontier(O.PLUS_TIMES_F32, A, F, xv, xv, sc, 1.0, 0.0)
    for h in (F, A, B, xv, sc):
        h.free()
