"""(or,and) on packed bits on the GPU: sh_bits_spmv, sh_bits_iterate, sh_bits_from_column / sh_bits_to_column through the
Python face, against the CPU oracle, the single-source path (sh_spmv / sh_iterate), the multi-vector path
(sh_iterate_multi), the reference's own BFS result and a plain numpy BFS.  Every matrix is uploaded with plan=1: the
packed kernels run on the CSR-stream plan's arrays.

Everything here is bit for bit: the semiring has the values 0 and 1 and OR is order-free, so there is no tolerance.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import golden, mtx
from oracle import oracle as O
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

WORDS = [1, 2, 4, 8]
SR = O.OR_AND_I32


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def pack(columns, n, words):
    """0/1 columns (None: all zero), at most 32 * words of them -> the (n, words) uint32 array: source s is bit s % 32 of word s // 32."""
    P = np.zeros((n, words), np.uint32)
    for s, c in enumerate(columns):
        if c is not None:
            P[:, s // 32] |= (np.asarray(c) != 0).astype(np.uint32) << np.uint32(s % 32)
    return P


def column(P, s):
    return ((P[:, s // 32] >> np.uint32(s % 32)) & np.uint32(1)).astype(np.int32)


def one_hot(n, v):
    x = np.zeros(n, np.int32)
    if v is not None:
        x[v] = 1
    return x


def oracle_runs(rp, ci, va, starts, y0s, a, b, cap):
    """O.iterate for every start vector (the oracle is a C library: the calls run side by side)."""
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(lambda xy: O.iterate(SR, rp, ci, va, xy[0], xy[1], a, b, 1e-4, cap), zip(starts, y0s)))


# ------------------------------------------------------------------ 1. one launch
def ragged_csr(seed, rows, cols, long_len):
    """Empty rows, short and medium rows, rows a whole wave takes, ONE row longer than the schedule's long-row threshold
    (4096 entries), column indices outside [0, cols) on both sides, explicit zero values, rows != cols."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 12, rows)
    deg[rng.random(rows) < 0.3] = 0
    deg[rng.integers(0, rows, 40)] = rng.integers(17, 300, 40)
    deg[rows // 3] = long_len
    deg[0] = 0
    deg[rows - 1] = 5
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, cols, rp[-1]).astype(np.int32)
    oob = rng.random(rp[-1]) < 0.03
    ci[oob] = np.where(rng.random(oob.sum()) < 0.5, -1 - rng.integers(0, 5, oob.sum()), cols + rng.integers(0, 1000, oob.sum()))
    va = rng.integers(0, 3, rp[-1]).astype(np.int32)   # a third of the stored values are 0
    return rp, ci, va, rng


def check_one_launch(eng, rows, cols, rp, ci, va, words, rng, density):
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    n_src = 32 * words
    X = (rng.random((cols, n_src)) < density).astype(np.int32)
    Y = (rng.random((rows, n_src)) < 0.3).astype(np.int32)
    PX, PY = pack(X.T, cols, words), pack(Y.T, rows, words)
    xv, yv, out = eng.vector(PX), eng.vector(PY), eng.alloc(rows * words)
    x1, y1, o1 = eng.alloc(cols), eng.alloc(rows), eng.alloc(rows)
    for alpha, beta in ((1, 0), (1, 1), (0, 1), (0, 0)):
        out.fill(0xdeadbeef, np.uint32)
        ns = eng.bits_spmv(A, xv, yv if beta else None, alpha, beta, out, words, timed=True)
        assert ns > 0
        got = out.download(np.uint32, shape=(rows, words))
        for s in range(n_src):
            xs, ys = np.ascontiguousarray(X[:, s]), np.ascontiguousarray(Y[:, s])
            want = O.kernel(SR, rp, ci, va, xs, ys, alpha, beta, vlength=cols)
            np.testing.assert_array_equal(column(got, s), want, err_msg=f"source {s} vs the oracle, alpha {alpha} beta {beta}")
            x1.upload(xs)
            y1.upload(ys)
            eng.spmv(SR, A, x1, y1, alpha, beta, o1)
            np.testing.assert_array_equal(column(got, s), o1.download(np.int32), err_msg=f"source {s} vs sh_spmv, alpha {alpha} beta {beta}")
    for v in (xv, yv, out, x1, y1, o1):
        v.free()
    A.free()


@pytest.mark.parametrize("words", WORDS)
def test_one_launch_on_reference_matrices(eng, matrix_name, words):
    rows, cols, _, rp, ci, va = H.mm_load(mtx(matrix_name), elem_is_int=True)
    check_one_launch(eng, rows, cols, rp, ci, va, words, np.random.default_rng(11 + words), density=0.05)


@pytest.mark.parametrize("words", WORDS)
def test_one_launch_on_ragged_matrix(eng, words):
    rows, cols = 3001, 2500
    rp, ci, va, rng = ragged_csr(300 + words, rows, cols, long_len=20_001)   # three segments and the fix-up
    assert (va == 0).any() and (ci < 0).any() and (ci >= cols).any() and (np.diff(rp) == 0).any() and np.diff(rp).max() > 4096
    # sparse x: a set bit in a long row's result then hangs on few entries, in whatever segment they sit
    check_one_launch(eng, rows, cols, rp, ci, va, words, rng, density=0.0005)


# ------------------------------------------------------------------ 2. iteration
def pick_sources(n, words):
    """Vertex 0 as source 0, then the first 32 * words - 1 of a seeded permutation of the others (all where n is smaller);
    None for the bits that are left (an all-zero start vector)."""
    rest = [int(v) for v in np.random.default_rng(7).permutation(np.arange(1, n))[:32 * words - 1]]
    srcs = [0] + rest
    return srcs + [None] * (32 * words - len(srcs))


def run_bits_iterate(eng, A, n, words, P0, a, b, cap, counts=False):
    xv, yv, sc = eng.vector(P0), eng.vector(P0), eng.alloc(n * words).fill(0)
    res = eng.bits_iterate(A, xv, yv, sc, a, b, words, max_iters=cap, counts=counts)
    got = xv.download(np.uint32, shape=(n, words))
    for v in (xv, yv, sc):
        v.free()
    return got, res


def check_iteration(eng, rp, ci, va, n, words, gold_final=None, gold_meta=None):
    sources = pick_sources(n, words)
    starts = [one_hot(n, s) for s in sources]
    P0 = pack(starts, n, words)
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    for a, b in ((1, 0), (1, 1)):
        full = oracle_runs(rp, ci, va, starts, starts, a, b, 2000)
        counts = [r[1] for r in full]
        real = [c for c, s in zip(counts, sources) if s is not None]
        print(f"n {n} words {words} (alpha, beta) ({a}, {b}): counts of the sources {sorted(set(real))}")
        assert len(set(real)) >= 2, "every source needs the same number of launches: nothing would be frozen early"
        for cap in (2000, max(counts) - 1):
            if cap < 1:
                continue
            if cap == 2000:
                ref = full
            else:   # a run that ends within the cap is the same run; the others are cut short
                late = [j for j, c in enumerate(counts) if c > cap]
                cut = oracle_runs(rp, ci, va, [starts[j] for j in late], [starts[j] for j in late], a, b, cap)
                ref = list(full)
                for j, r in zip(late, cut):
                    ref[j] = r
                assert late and not any(r[2] for r in cut)
            got, (launches, iters, conv, per, total) = run_bits_iterate(eng, A, n, words, P0, a, b, cap)
            assert iters == [r[1] for r in ref], (a, b, cap)
            assert conv == [r[2] for r in ref], (a, b, cap)
            assert launches == max(iters) and len(per) == launches and total == sum(per)
            for s in range(32 * words):
                np.testing.assert_array_equal(column(got, s), (ref[s][0] != 0).astype(np.int32),
                                              err_msg=f"source bit {s} (vertex {sources[s]}), alpha {a} beta {b}, max_iters {cap}")
            if cap == 2000 and (a, b) == (1, 0) and gold_final is not None:   # vertex 0 is source 0: the reference's own run
                np.testing.assert_array_equal(column(got, 0), (gold_final != 0).astype(np.int32))
                assert [iters[0], int(conv[0])] == gold_meta.tolist()
    A.free()


@pytest.mark.parametrize("words", [1, 4])
def test_iteration_on_reference_matrices(eng, matrix_name, words):
    g = golden(matrix_name)
    rows, cols, _, rp, ci, va = H.mm_load(mtx(matrix_name), elem_is_int=True)
    check_iteration(eng, rp, ci, va, rows, words, g["bfs_final"], g["bfs_meta"])


@pytest.mark.parametrize("words", WORDS)
def test_iteration_on_rmat16(eng, words):
    rp, ci, va = H.rmat(16, seed=40)
    check_iteration(eng, rp, ci, va.astype(np.int32), 1 << 16, words)


# ------------------------------------------------------------------ 3. the same as sh_iterate_multi at width 32
@pytest.mark.parametrize("ab", [(1, 0), (1, 1)])
def test_words_1_equals_iterate_multi_width_32(eng, ab):
    a, b = ab
    n = 1 << 16
    rp, ci, va = H.rmat(16, seed=40)
    va = va.astype(np.int32)
    sources = pick_sources(n, 1)
    starts = [one_hot(n, s) for s in sources]
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    X0 = np.ascontiguousarray(np.stack(starts, axis=1))
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * 32).fill(0)
    m_launches, m_iters, m_conv, _, _ = eng.iterate_multi(SR, A, xv, yv, sc, a, b, 32, max_iters=2000)
    want = xv.download(np.int32, shape=(n, 32))
    for v in (xv, yv, sc):
        v.free()
    bv, by, bs, col = eng.vector(pack(starts, n, 1)), eng.vector(pack(starts, n, 1)), eng.alloc(n).fill(0), eng.alloc(n)
    launches, iters, conv, _, _ = eng.bits_iterate(A, bv, by, bs, a, b, 1, max_iters=2000)
    assert (launches, iters, conv) == (m_launches, m_iters, m_conv)
    assert len(set(iters)) >= 2
    for s in range(32):
        eng.bits_to_column(bv, n, 1, s, col)
        np.testing.assert_array_equal(col.download(np.int32), want[:, s], err_msg=f"source {s}")
    for v in (bv, by, bs, col):
        v.free()
    A.free()


# ------------------------------------------------------------------ 4. level counts
def bfs_levels(rp, ci, va, n, source):
    """levels[d] = number of vertices at distance d >= 1 from `source`: row r is reached from column c through a stored
    entry (r, c) with a non-zero value and 0 <= c < n."""
    r_e = np.repeat(np.arange(n), np.diff(rp))
    ok = (va != 0) & (ci >= 0) & (ci < n)
    r_e, c_e = r_e[ok], ci[ok]
    seen = np.zeros(n, bool)
    seen[source] = True
    front, levels = seen.copy(), [0]
    while True:
        hit = np.zeros(n, bool)
        hit[r_e[front[c_e]]] = True
        front = hit & ~seen
        if not front.any():
            return levels
        levels.append(int(front.sum()))
        seen |= front


def check_level_counts(eng, rp, ci, va, n, words):
    sources = pick_sources(n, words)
    P0 = pack([one_hot(n, s) for s in sources], n, words)
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    plain, (launches, iters, conv, _, _) = run_bits_iterate(eng, A, n, words, P0, 1, 1, 2000)
    got, (c_launches, c_iters, c_conv, _, _, newly) = run_bits_iterate(eng, A, n, words, P0, 1, 1, 2000, counts=True)
    np.testing.assert_array_equal(got, plain)
    assert (c_launches, c_iters, c_conv) == (launches, iters, conv) and all(conv)
    assert newly.shape == (launches, 32 * words) and newly.dtype == np.uint32
    for s, v in enumerate(sources):
        want = np.zeros(launches, np.uint32)
        if v is not None:
            lv = bfs_levels(rp, ci, va, n, v)
            assert iters[s] == len(lv), f"source {s}: the launch after the last level confirms"
            want[:len(lv) - 1] = lv[1:]
        np.testing.assert_array_equal(newly[:, s], want, err_msg=f"source bit {s} (vertex {v})")
        assert not newly[iters[s] - 1:, s].any()   # frozen: nothing afterwards
    A.free()
    return iters


@pytest.mark.parametrize("words", WORDS)
def test_level_counts_equal_a_plain_bfs_on_rmat12(eng, words):
    rp, ci, va = H.rmat(12, seed=3)
    iters = check_level_counts(eng, rp, ci, va.astype(np.int32), 1 << 12, words)
    assert len(set(iters)) >= 2, "the sources were meant to freeze at different launches"


@pytest.mark.parametrize("words", [1, 8])
def test_level_counts_with_long_rows_zero_values_and_stray_columns(eng, words):
    n = 3001
    rp, ci, va, _ = ragged_csr(500 + words, n, n, long_len=9_000)   # two segments and the fix-up
    check_level_counts(eng, rp, ci, va, n, words)


def test_level_counts_on_a_reference_matrix(eng):
    rows, _, _, rp, ci, va = H.mm_load(mtx("matrix"), elem_is_int=True)
    check_level_counts(eng, rp, ci, va, rows, 2)


# ------------------------------------------------------------------ 5. pack / unpack
def test_columns_round_trip_and_leave_other_bits_alone(eng):
    n, words = 1000 + 37, 8   # not a multiple of 64
    rng = np.random.default_rng(5)
    P = rng.integers(0, 1 << 32, (n + 3, words), dtype=np.uint64).astype(np.uint32)
    B, v, back = eng.vector(P), eng.alloc(n + 3), eng.alloc(n + 3)
    for s in range(32 * words):
        c = rng.integers(0, 2, n).astype(np.int32) * rng.integers(1, 1000, n).astype(np.int32)   # any non-zero value sets the bit
        v.upload(np.concatenate([c, [1, 1, 1]]).astype(np.int32))
        eng.bits_from_column(v, n, words, s, B)
        want = P.copy()
        bit = np.uint32(1) << np.uint32(s % 32)
        want[:n, s // 32] = (P[:n, s // 32] & ~bit) | ((c != 0).astype(np.uint32) << np.uint32(s % 32))
        got = B.download(np.uint32, shape=(n + 3, words))
        np.testing.assert_array_equal(got, want, err_msg=f"source {s}: another bit, or a vertex past n, changed")
        P = want
        back.fill(7, np.int32)
        eng.bits_to_column(B, n, words, s, back)
        res = back.download(np.int32)
        np.testing.assert_array_equal(res[:n], (c != 0).astype(np.int32))
        assert res[n:].tolist() == [7, 7, 7]
    for x in (B, v, back):
        x.free()


@pytest.mark.parametrize("words", [1, 8])
def test_packed_iteration_of_columns_equals_sh_iterate(eng, words):
    n = 1 << 12
    rp, ci, va = H.rmat(12, seed=3)
    va = va.astype(np.int32)
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    picks = {0: 0, 32 * words - 1: 77, 5: 1234}   # source bit -> start vertex
    B = eng.alloc(n * words).fill(0, np.uint32)
    col = eng.alloc(n)
    for s, v in picks.items():
        col.upload(one_hot(n, v))
        eng.bits_from_column(col, n, words, s, B)
    Y = eng.vector(B.download(np.uint32))
    sc = eng.alloc(n * words).fill(0)
    launches, iters, conv, _, _ = eng.bits_iterate(A, B, Y, sc, 1, 0, words, max_iters=2000)
    for s, v in picks.items():
        xv, yv, s1 = eng.vector(one_hot(n, v)), eng.vector(one_hot(n, v)), eng.alloc(n).fill(0)
        it, cv, _, _ = eng.iterate(SR, A, xv, yv, s1, 1, 0, max_iters=2000)
        eng.bits_to_column(B, n, words, s, col)
        np.testing.assert_array_equal(col.download(np.int32), (xv.download(np.int32) != 0).astype(np.int32), err_msg=f"source {s}")
        assert (iters[s], conv[s]) == (it, cv)
        for x in (xv, yv, s1):
            x.free()
    for x in (B, Y, sc, col):
        x.free()
    A.free()


# ------------------------------------------------------------------ 6. errors, nothing to do
def test_errors(eng):
    rp, ci, va = H.rmat(12, seed=3)
    va = va.astype(np.int32)
    n, words = 1 << 12, 2
    At = eng.upload_csr(n, n, rp, ci, va.astype(np.float32), plan=2)
    assert At.plan()[0] == "tiled"
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    R = eng.upload_csr(n - 1, n, rp[:-1], ci[:rp[-2]], va[:rp[-2]], plan=1)   # not square
    X, out, short = eng.alloc(n * words).fill(1, np.uint32), eng.alloc(n * words).fill(0), eng.alloc(n * words - 1)

    def refused(code, word, fn, *args, **kw):
        with pytest.raises(EngineError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code and str(ei.value) and word in str(ei.value), (ei.value.code, str(ei.value))

    refused(abi.SH_EINVAL, "plan = 1", eng.bits_spmv, At, X, None, 1, 0, out, words)
    refused(abi.SH_EINVAL, "plan = 1", eng.bits_iterate, At, X, X, out, 1, 0, words)
    for w in (0, 3, 16):
        refused(abi.SH_EINVAL, "words", eng.bits_spmv, A, X, None, 1, 0, out, w)
        refused(abi.SH_EINVAL, "words", eng.bits_iterate, A, X, X, out, 1, 0, w)
        refused(abi.SH_EINVAL, "words", eng.bits_from_column, X, 8, w, 0, out)
        refused(abi.SH_EINVAL, "words", eng.bits_to_column, X, 8, w, 0, out)
    for s in (-1, 32 * words):
        refused(abi.SH_EINVAL, "source", eng.bits_from_column, X, 8, words, s, out)
        refused(abi.SH_EINVAL, "source", eng.bits_to_column, X, 8, words, s, out)
    refused(abi.SH_ESHAPE, "", eng.bits_spmv, A, X, None, 1, 0, short, words)
    refused(abi.SH_ESHAPE, "", eng.bits_spmv, A, short, None, 1, 0, out, words)
    refused(abi.SH_ESHAPE, "", eng.bits_spmv, A, X, short, 1, 1, out, words)
    refused(abi.SH_ESHAPE, "", eng.bits_iterate, A, X, short, out, 1, 0, words)       # Y0 is read whatever beta is
    refused(abi.SH_ESHAPE, "", eng.bits_iterate, A, X, X, short, 1, 0, words)
    refused(abi.SH_ESHAPE, "square", eng.bits_iterate, R, X, X, out, 1, 0, words)
    refused(abi.SH_ESHAPE, "", eng.bits_from_column, short, n, words, 0, short)       # B too short for n * words
    refused(abi.SH_ESHAPE, "", eng.bits_to_column, short, n, words, 0, X)
    refused(abi.SH_EINVAL, "alias", eng.bits_spmv, A, X, None, 1, 0, X, words)
    refused(abi.SH_EINVAL, "alias", eng.bits_iterate, A, X, out, X, 1, 0, words)
    refused(abi.SH_EINVAL, "NULL", eng.bits_spmv, A, X, None, 1, 1, out, words)         # beta != 0 reads Y
    refused(abi.SH_EINVAL, "NULL", eng.bits_iterate, A, X, None, out, 1, 0, words)
    # max_iters <= 0: nothing runs, nothing is an error
    for cap in (0, -3):
        res = eng.bits_iterate(A, X, X, out, 1, 0, words, max_iters=cap, counts=True)
        assert res[:5] == (0, [0] * 64, [False] * 64, [], 0) and res[5].shape == (0, 64)
    assert (X.download(np.uint32) == 1).all()
    # and the engine still works
    P = pack([one_hot(n, 0), np.ones(n, np.int32)], n, words)
    X.upload(P)
    eng.bits_spmv(A, X, None, 1, 0, out, words)
    got = out.download(np.uint32, shape=(n, words))
    np.testing.assert_array_equal(column(got, 0), O.kernel(SR, rp, ci, va, one_hot(n, 0), np.zeros(n), 1, 0))
    np.testing.assert_array_equal(column(got, 1), O.kernel(SR, rp, ci, va, np.ones(n), np.zeros(n), 1, 0))
    for v in (X, out, short):
        v.free()
    for m in (A, At, R):
        m.free()


def test_matrix_without_rows_launches_nothing(eng):
    A = eng.upload_csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), plan=1)
    X, out = eng.alloc(8).fill(1, np.uint32), eng.alloc(8).fill(7, np.uint32)
    assert eng.bits_spmv(A, X, None, 1, 0, out, 4) is None      # SH_OK
    launches, iters, conv, _, _ = eng.bits_iterate(A, X, X, out, 1, 0, 4, max_iters=5)
    eng.synchronize()
    assert out.download(np.uint32).tolist() == [7] * 8 and X.download(np.uint32).tolist() == [1] * 8
    # no row changes anything: every source is confirmed by the first (empty) launch, as sh_iterate reports it
    assert (launches, iters, conv) == (1, [1] * 128, [True] * 128)
    A.free()
    # rows without a single entry: the identity through the epilogue, for every bit
    A = eng.upload_csr(5, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), plan=1)
    Yh = np.arange(20, dtype=np.uint32) * np.uint32(0x01010101)
    X, Y, out = eng.alloc(20).fill(0xffffffff, np.uint32), eng.vector(Yh), eng.alloc(20).fill(7, np.uint32)
    eng.bits_spmv(A, X, Y, 1, 1, out, 4)
    assert out.download(np.uint32).tolist() == Yh.tolist()
    eng.bits_spmv(A, X, None, 1, 0, out, 4)
    assert out.download(np.uint32).tolist() == [0] * 20
    A.free()


# ------------------------------------------------------------------ 7. no growth of device memory
def test_repeated_create_iterate_free_does_not_grow_device_memory(eng):
    """200 cycles of upload, iterate (with and without counts) and free.  A cycle allocates a matrix and three vectors of
    128 KB; leaking any one of the vectors every cycle would take 25 MB, all of them and the matrix over 100 MB.  The
    free-memory reading is the device's, so 16 MB are allowed for what else happens on it (tools/leak_check.py allows 64)."""
    n, words = 1 << 12, 8
    rp, ci, va = H.rmat(12, seed=3)
    va = va.astype(np.int32)
    P0 = pack([one_hot(n, s) for s in pick_sources(n, words)], n, words)

    def cycle(counts):
        A = eng.upload_csr(n, n, rp, ci, va, plan=1)
        xv, yv, sc = eng.vector(P0), eng.vector(P0), eng.alloc(n * words)
        res = eng.bits_iterate(A, xv, yv, sc, 1, 1, words, max_iters=100, counts=counts)
        for v in (xv, yv, sc):
            v.free()
        A.free()
        return res[0]

    first = cycle(True)   # (loads the code object, allocates the engine's iteration state once)
    eng.synchronize()
    before = eng.max_alloc()
    for i in range(200):
        assert cycle(i % 2 == 0) == first
    eng.synchronize()
    after = eng.max_alloc()
    print(f"free device memory before {before >> 20} MiB, after {after >> 20} MiB")
    assert before - after < (16 << 20), (before, after)
