"""Several vectors per launch on the GPU: sh_spmm and sh_iterate_multi through the Python face, against the golden
vectors of the real reference, the single-vector path (sh_spmv / sh_iterate) and the CPU oracle.  Every matrix is
uploaded with plan=1: the multi-vector kernels run on the CSR-stream plan's arrays.

Bounds.  Integer-valued (+,x) data and the three order-free semirings: bit for bit.  General floats: rows of at most 64
entries drawn from [0.5, 1.5), every element within REL * max(1, |want|) of the gold sum -- with positive terms a
sequential and a tree sum of n <= 64 floats each stay within (n-1) * 2^-24 relative of the exact sum, so the two
differ by less than 7.6e-6 < REL whatever the order.  That is this file's general-float case only: (+,x) on mixed signs,
wide dynamic range, rows through the wave sums, the long-row segments and their fix-up, the alpha / beta / Y epilogue and
non-finite inputs is held to a derived float32 bound against float64 in tests/test_float_gpu.py (bound: tests/float_ref.py).
"""
import numpy as np
import pytest

from conftest import golden, mtx
from oracle import oracle as O
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

REL = 1e-5   # the project's tolerance for float SpMV (tests/test_parity_gpu.py)
WIDTHS = [4, 8, 16, 32]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def interleave(columns, dt):
    """k vectors -> the (n, k) C-contiguous array sh_spmm reads: element i of vector j at i*k + j."""
    return np.ascontiguousarray(np.stack([np.asarray(c, dt) for c in columns], axis=1))


def run_spmm(eng, sr, A, rows, X, Y, alpha, beta):
    dt = O.elem_dtype(sr)
    k = X.shape[1]
    xv = eng.vector(np.ascontiguousarray(X, dt))
    yv = None if Y is None else eng.vector(np.ascontiguousarray(Y, dt))
    out = eng.alloc(rows * k).fill(0)
    ns = eng.spmm(sr, A, xv, yv, alpha, beta, out, k, timed=True)
    res = out.download(dt, shape=(rows, k))
    for v in (xv, yv, out):
        if v is not None:
            v.free()
    assert ns > 0
    return res


def run_spmv(eng, sr, A, rows, x, y, alpha, beta):
    dt = O.elem_dtype(sr)
    xv = eng.vector(np.ascontiguousarray(x, dt))
    yv = None if y is None else eng.vector(np.ascontiguousarray(y, dt))
    out = eng.alloc(rows).fill(0)
    eng.spmv(sr, A, xv, yv, alpha, beta, out)
    res = out.download(dt)
    for v in (xv, yv, out):
        if v is not None:
            v.free()
    return res


# ------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("width", WIDTHS)
def test_golden_columns_match_reference_bit_for_bit(eng, matrix_name, width):
    g = golden(matrix_name)
    rows, cols, _, rp, ci, va = H.mm_load(mtx(matrix_name))
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    x1 = np.ones(cols, np.float32)
    xm = (1 + np.arange(cols) % 7).astype(np.float32)
    ym = (np.arange(rows) % 5).astype(np.float32)
    X = interleave([x1 if j % 2 == 0 else xm for j in range(width)], np.float32)
    got = run_spmm(eng, O.PLUS_TIMES_F32, A, rows, X, None, 1.0, 0.0)
    for j in range(width):
        want = g["gold_x1"] if j % 2 == 0 else g["gold_xmod"]
        np.testing.assert_array_equal(bits(got[:, j]), bits(want), err_msg=f"column {j}")
    Y = interleave([ym] * width, np.float32)
    got = run_spmm(eng, O.PLUS_TIMES_F32, A, rows, X, Y, 2.0, 0.5)
    for j in range(1, width, 2):
        np.testing.assert_array_equal(bits(got[:, j]), bits(g["kern_spmv_ab"]), err_msg=f"column {j}")
    A.free()


# ------------------------------------------------------------------ 2. the order-free semirings: same bits as sh_spmv
def ragged_csr(seed, rows, cols, long_len):
    """Empty rows, short and medium rows, ONE row longer than the schedule's long-row threshold (4096 entries), and
    column indices outside [0, cols) on both sides."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 12, rows)
    deg[rng.random(rows) < 0.3] = 0
    deg[rng.integers(0, rows, 40)] = rng.integers(17, 300, 40)     # rows a whole wave sums
    deg[rows // 3] = long_len
    deg[0] = 0
    deg[rows - 1] = 5
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, cols, rp[-1]).astype(np.int32)
    oob = rng.random(rp[-1]) < 0.03
    ci[oob] = np.where(rng.random(oob.sum()) < 0.5, -1 - rng.integers(0, 5, oob.sum()), cols + rng.integers(0, 1000, oob.sum()))
    return rp, ci, rng


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("sr", [O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32])
def test_column_equals_single_vector_path_and_oracle(eng, sr, width):
    rows, cols = 3001, 2500
    rp, ci, rng = ragged_csr(100 + sr, rows, cols, long_len=20_001)   # three segments and the fix-up
    dt = O.elem_dtype(sr)
    if sr == O.MIN_PLUS_F32:
        va = rng.integers(1, 17, rp[-1]).astype(dt)
        cols_x = [np.where(rng.random(cols) < 0.5, O.FLT_MAX, rng.integers(0, 40, cols)).astype(dt) for _ in range(width)]
        cols_y = [rng.integers(0, 50, rows).astype(dt) for _ in range(width)]
        alpha, beta = 2.0, 1.0
    elif sr == O.OR_AND_I32:
        va = rng.integers(0, 2, rp[-1]).astype(dt)
        cols_x = [(rng.random(cols) < 0.02 * (j + 1)).astype(dt) for j in range(width)]
        cols_y = [rng.integers(0, 2, rows).astype(dt) for _ in range(width)]
        alpha, beta = 1, 1
    else:
        va = rng.integers(-1000, 1000, rp[-1]).astype(dt)
        cols_x = [rng.integers(-1000, 1000, cols).astype(dt) for _ in range(width)]
        cols_y = [rng.integers(-1000, 1000, rows).astype(dt) for _ in range(width)]
        alpha, beta = 500, -200
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    got = run_spmm(eng, sr, A, rows, interleave(cols_x, dt), interleave(cols_y, dt), alpha, beta)
    for j in range(width):
        single = run_spmv(eng, sr, A, rows, cols_x[j], cols_y[j], alpha, beta)
        np.testing.assert_array_equal(bits(got[:, j]), bits(single), err_msg=f"column {j} vs sh_spmv")
        want = O.kernel(sr, rp, ci, va, cols_x[j], cols_y[j], alpha, beta, vlength=cols)
        np.testing.assert_array_equal(bits(got[:, j]), bits(want), err_msg=f"column {j} vs the oracle")
    A.free()


# ------------------------------------------------------------------ 3. general floats
@pytest.mark.parametrize("width", WIDTHS)
def test_general_floats_within_rel_of_gold(eng, width):
    rng = np.random.default_rng(77 + width)
    rows, cols = 20_000, 17_000
    deg = rng.integers(0, 65, rows)            # rows of at most 64 entries: see the module docstring
    deg[::97] = 64
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, cols, rp[-1]).astype(np.int32)
    va = rng.uniform(0.5, 1.5, rp[-1]).astype(np.float32)
    cols_x = [rng.uniform(0.5, 1.5, cols).astype(np.float32) for _ in range(width)]
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    got = run_spmm(eng, O.PLUS_TIMES_F32, A, rows, interleave(cols_x, np.float32), None, 1.0, 0.0)
    for j in range(width):
        want = O.gold_spmv(rp, ci, va, cols_x[j]).astype(np.float64)
        err = np.abs(got[:, j].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        print(f"width {width} column {j}: worst error {err.max():.3e} of the bound {REL:.0e}")
        assert not (err > REL).any(), f"column {j}: {(err > REL).sum()} elements off, worst {err.max():.3e}"
    A.free()


# ------------------------------------------------------------------ 4. multi-source iteration
def start_vector(sr, n, source):
    """x0 == y0 of the SSSP / BFS apps (O.initial_vector) with `source` in the place of vertex 0."""
    v = np.full(n, O.FLT_MAX, np.float32) if sr == O.MIN_PLUS_F32 else np.zeros(n, np.int32)
    v[source] = 0.0 if sr == O.MIN_PLUS_F32 else 1
    return v


def choose_sources(sr, rp, ci, va, n, width, a, b):
    """`width` distinct vertices, vertex 0 first, whose single-source runs on the CPU oracle do not all take the same
    number of launches.  -> (sources, [(final, iters, converged)] per source)"""
    rng = np.random.default_rng(7)
    cands = [0] + [int(v) for v in rng.permutation(np.arange(1, n))[:3 * width]]
    runs = {}
    for s in cands:
        x0 = start_vector(sr, n, s)
        runs[s] = O.iterate(sr, rp, ci, va, x0, x0, a, b, 1e-4, 2000)
        if len(runs) >= width and len({r[1] for r in runs.values()}) >= 2:
            break
    other = next((s for s in runs if runs[s][1] != runs[0][1]), None)
    assert other is not None, "every candidate source needs the same number of launches: nothing would be frozen early"
    chosen = [0, other] + [s for s in runs if s not in (0, other)]
    chosen = chosen[:width]
    return chosen, [runs[s] for s in chosen]


def check_multi_source(eng, sr, rp, ci, va, n, width, gold_final=None, gold_meta=None):
    dt = O.elem_dtype(sr)
    a, b = (0.0, 0.0) if sr == O.MIN_PLUS_F32 else (1, 0)
    sources, want = choose_sources(sr, rp, ci, va, n, width, a, b)
    counts = [w[1] for w in want]
    assert len(set(counts)) >= 2
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    X0 = interleave([start_vector(sr, n, s) for s in sources], dt)
    for cap in (2000, max(counts) - 1):
        if cap < 1:
            continue
        xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0)
        launches, iters, conv, per, total = eng.iterate_multi(sr, A, xv, yv, sc, a, b, width, delta=1e-4, max_iters=cap)
        got = xv.download(dt, shape=(n, width))
        for v in (xv, yv, sc):
            v.free()
        if cap == 2000:
            ref = want
        else:
            ref = [O.iterate(sr, rp, ci, va, start_vector(sr, n, s), start_vector(sr, n, s), a, b, 1e-4, cap) for s in sources]
            assert [r[2] for r in ref] == [c <= cap for c in counts] and not all(r[2] for r in ref)
        assert iters == [r[1] for r in ref], (sources, cap)
        assert conv == [r[2] for r in ref], (sources, cap)
        assert launches == max(iters) and len(per) == launches and total == sum(per)
        for j in range(width):
            np.testing.assert_array_equal(bits(got[:, j]), bits(ref[j][0]), err_msg=f"source {sources[j]} (column {j}), max_iters {cap}")
        if cap == 2000 and gold_final is not None:   # vertex 0 is column 0: the reference's own run
            np.testing.assert_array_equal(bits(got[:, 0]), bits(gold_final))
            assert [iters[0], int(conv[0])] == gold_meta.tolist()
    A.free()


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("sr,tag", [(O.MIN_PLUS_F32, "sssp"), (O.OR_AND_I32, "bfs")])
def test_multi_source_iteration_on_reference_matrices(eng, matrix_name, sr, tag, width):
    g = golden(matrix_name)
    rows, cols, _, rp, ci, va = H.mm_load(mtx(matrix_name), elem_is_int=(sr == O.OR_AND_I32))
    check_multi_source(eng, sr, rp, ci, va, rows, width, g[tag + "_final"], g[tag + "_meta"])


@pytest.mark.parametrize("sr,width", [(O.MIN_PLUS_F32, 8), (O.OR_AND_I32, 32)])
def test_multi_source_iteration_on_rmat16(eng, sr, width):
    rp, ci, va = H.rmat(16, seed=40)
    check_multi_source(eng, sr, rp, ci, va.astype(O.elem_dtype(sr)), 1 << 16, width)


def test_pagerank_style_columns_freeze_like_single_runs(eng):
    """(+,x) with delta = 1e-4: a fixed point that is approached, not hit.  Every column stops where its single run stops."""
    width = 4
    rows, cols, _, rp, ci, va = H.mm_load(mtx("matrix2"), normalise=H.NORM_PAGERANK, damping=0.85)
    n = rows
    rng = np.random.default_rng(9)
    one_hot = np.zeros(n, np.float32)
    one_hot[3] = 1.0
    starts = [np.full(n, np.float32(1.0) / np.float32(n), np.float32),   # the app's start
              one_hot,
              (rng.random(n) / n).astype(np.float32),
              np.full(n, np.float32(50.0) / np.float32(n), np.float32)]
    y0 = np.ones(n, np.float32)
    beta = (np.float32(1.0) - np.float32(0.85)) / np.float32(n)
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    single = []
    for x0 in starts:
        xv, yv, sc = eng.vector(x0), eng.vector(y0), eng.alloc(n).fill(0)
        it, conv, _, _ = eng.iterate(O.PLUS_TIMES_F32, A, xv, yv, sc, 1.0, beta, delta=1e-4, max_iters=2000)
        single.append((xv.download(np.float32), it, conv))
        for v in (xv, yv, sc):
            v.free()
    assert len({s[1] for s in single}) >= 2, "the start vectors were meant to need different numbers of launches"
    xv, yv, sc = eng.vector(interleave(starts, np.float32)), eng.vector(interleave([y0] * width, np.float32)), eng.alloc(n * width).fill(0)
    launches, iters, conv, _, _ = eng.iterate_multi(O.PLUS_TIMES_F32, A, xv, yv, sc, 1.0, beta, width, delta=1e-4, max_iters=2000)
    got = xv.download(np.float32, shape=(n, width))
    assert iters == [s[1] for s in single] and conv == [s[2] for s in single] and launches == max(iters)
    for j in range(width):
        want = single[j][0].astype(np.float64)
        assert not (np.abs(got[:, j] - want) > REL * np.maximum(1.0, np.abs(want))).any(), f"column {j} vs sh_iterate"
        want, w_it, w_conv = O.iterate(O.PLUS_TIMES_F32, rp, ci, va, starts[j], y0, 1.0, beta, 1e-4, 2000)
        assert not (np.abs(got[:, j] - want.astype(np.float64)) > REL * np.maximum(1.0, np.abs(want))).any(), f"column {j} vs the oracle"
    for v in (xv, yv, sc):
        v.free()
    A.free()


# ------------------------------------------------------------------ 5. errors
def test_errors(eng):
    rp, ci, va = H.rmat(12, seed=3)
    n = 1 << 12
    At = eng.upload_csr(n, n, rp, ci, va, plan=2)
    assert At.plan()[0] == "tiled"
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    X, out, short = eng.alloc(n * 8).fill(1.0), eng.alloc(n * 8).fill(0), eng.alloc(n * 8 - 1)
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.PLUS_TIMES_F32, At, X, None, 1.0, 0.0, out, 8)
    assert ei.value.code == abi.SH_EINVAL and "plan = 1" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng.iterate_multi(O.MIN_PLUS_F32, At, X, X, out, 0.0, 0.0, 8)
    assert ei.value.code == abi.SH_EINVAL and "plan = 1" in str(ei.value)
    for width in (3, 64):
        with pytest.raises(EngineError) as ei:
            eng.spmm(O.PLUS_TIMES_F32, A, X, None, 1.0, 0.0, out, width)
        assert ei.value.code == abi.SH_EINVAL and "width" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.PLUS_TIMES_F32, A, X, None, 1.0, 0.0, short, 8)
    assert ei.value.code == abi.SH_ESHAPE
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.PLUS_TIMES_F32, A, short, None, 1.0, 0.0, out, 8)
    assert ei.value.code == abi.SH_ESHAPE
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.MIN_PLUS_F32, A, X, short, 0.0, 0.0, out, 8)      # (min,+) reads Y
    assert ei.value.code == abi.SH_ESHAPE
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.PLUS_TIMES_F32, A, X, None, 1.0, 0.0, X, 8)
    assert ei.value.code == abi.SH_EINVAL and "alias" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        eng.spmm(O.MIN_PLUS_F32, A, X, None, 0.0, 0.0, out, 8)
    assert ei.value.code == abi.SH_EINVAL
    # max_iters <= 0: nothing runs, nothing is an error
    launches, iters, conv, per, total = eng.iterate_multi(O.MIN_PLUS_F32, A, X, X, out, 0.0, 0.0, 8, max_iters=0)
    assert (launches, iters, conv, per, total) == (0, [0] * 8, [False] * 8, [], 0)
    # and the engine still works
    eng.spmm(O.PLUS_TIMES_F32, A, X, None, 1.0, 0.0, out, 8)
    want = O.kernel(O.PLUS_TIMES_F32, rp, ci, va, np.ones(n, np.float32), np.zeros(n), 1.0, 0.0)
    np.testing.assert_array_equal(out.download(np.float32, shape=(n, 8))[:, 5], want)
    for v in (X, out, short):
        v.free()
    A.free()
    At.free()


# ------------------------------------------------------------------ 6. nothing to do
def test_matrix_without_rows_launches_nothing(eng):
    A = eng.upload_csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), plan=1)
    X, out = eng.alloc(4).fill(1.0), eng.alloc(4).fill(7.0)
    assert eng.spmm(O.PLUS_TIMES_F32, A, X, None, 1.0, 0.0, out, 4) is None      # SH_OK
    eng.synchronize()
    assert out.download(np.float32).tolist() == [7.0] * 4
    A.free()
    # rows without a single entry: the identity through the epilogue, for every column
    A = eng.upload_csr(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), plan=1)
    X, Y, out = eng.alloc(20).fill(1.0), eng.vector(np.arange(20, dtype=np.float32)), eng.alloc(20).fill(7.0)
    eng.spmm(O.PLUS_TIMES_F32, A, X, Y, 1.0, 2.0, out, 4)
    assert out.download(np.float32).tolist() == (2.0 * np.arange(20)).tolist()
    A.free()
