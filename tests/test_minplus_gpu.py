"""(min,+) on real weights, on the GPU.  Every product |x| + |a| is one rounding of its own and min over floats that are
not NaN is exact and order-free (tests/minplus_ref.py; tests/test_minplus_ref.py shows the sequential oracle and an
order-free numpy restatement agree bit for bit on these inputs), so EVERY path must give the oracle's bits on arbitrary
real inputs, whatever order it reduces in:

  a. sh_spmv under the five plan variants (stream; tiled with 4 / 8 / 16-bit codes, raw values, folded and not),
  b. dead-tile skipping with real coded weights and 0 / 1 / 6 / 2000 reached x words, around the 2^103 limit,
  c. sh_spmm at widths 4..32 through the one-team rows, the wave rows and the long-row fix-up,
  d. sh_iterate, sh_iterate_multi, sh_iterate_frontier and the sharded driver on a weighted R-MAT and a weighted grid:
     launch count, converged flag and vector bits of O.iterate; converged vectors inside the float64 path bound,
  e. Inf, subnormals, -0.0, -FLT_MAX, odd scalars, an Inf that never converges; NaN: rows that read none keep their bits.
Nothing here is compared with a tolerance taken from the device's output.
"""
import functools

import numpy as np
import pytest

import float_ref as F
import minplus_ref as M
from oracle import oracle as O
from sparseharness_amd.engine import Engine
from test_float_gpu import CODING, SP_COLS, C1, C2, R_SHORT, R_SHORT2, R_MID, R_LONG, special_pattern
from test_multi_gpu import interleave, run_spmm, run_spmv
from test_parity_gpu import clustered_matrix

pytestmark = pytest.mark.gpu

MP = O.MIN_PLUS_F32
FLT_MAX = M.FLT_MAX
bits = M.bits
WIDTHS = [4, 8, 16, 32]
PLANS = ["stream", "tiled", "tiled-8bit", "tiled-raw", "tiled-nofold"]
EXACT = 1e-300      # below every float32 difference: the loop stops at an exact fixed point


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(params=PLANS)
def plan(request, monkeypatch):
    """The plan variants of tests/test_parity_gpu.py's fixture; -> the variant's name."""
    monkeypatch.setenv("SH_PLAN", request.param.split("-")[0])
    monkeypatch.setenv("SH_VALCODE", {"raw": "off", "8bit": "8"}.get(request.param.split("-")[-1], "auto"))
    monkeypatch.setenv("SH_FOLD", "0" if request.param.endswith("nofold") else "1")
    return request.param


GENERATORS = M.generators(clustered_matrix)


@functools.lru_cache(maxsize=None)
def data(name):
    c = GENERATORS[name](width=32)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def expected(name, j, alpha, beta):
    """O.kernel on column j of the input set (-1: its x / y themselves)."""
    c = data(name)
    x, y = (c["x"], c["y"]) if j < 0 else (c["xs"][j], c["ys"][j])
    return O.kernel(MP, c["rp"], c["ci"], c["va"], x, y, alpha, beta, vlength=c["cols"])


def assert_bits(got, want, msg):
    bad = np.nonzero(bits(got) != bits(want))[0]
    assert len(bad) == 0, (f"{msg}: {len(bad)} of {len(want)} rows differ, first rows {bad[:8].tolist()}: got {got[bad[:8]]!r} "
                           f"({[hex(w) for w in bits(got)[bad[:8]]]}) want {want[bad[:8]]!r} ({[hex(w) for w in bits(want)[bad[:8]]]})")


def upload(eng, c, plan, **kw):
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], **kw)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    return A


# ------------------------------------------------------------------ a. sh_spmv, every plan, every value layout
@pytest.mark.parametrize("name", list(GENERATORS))
def test_spmv_equals_oracle_bit_for_bit(eng, plan, name):
    c = data(name)
    A = upload(eng, c, plan)
    if plan.startswith("tiled"):
        # the few-values inputs take the coded layout they were made for; wide_range weights are all different: raw
        assert f"values={CODING.get((name, plan), 'raw')}" in A.describe(), A.describe()
    for j in (-1, 0, 1):                                   # three x through one uploaded matrix
        x, y = (c["x"], c["y"]) if j < 0 else (c["xs"][j], c["ys"][j])
        for alpha, beta in M.EPILOGUES:
            got = run_spmv(eng, MP, A, c["rows"], x, y, alpha, beta)
            assert_bits(got, expected(name, j, alpha, beta), f"sh_spmv {name} {plan} x{j} alpha={alpha:g} beta={beta:g}")
    A.free()


# ------------------------------------------------------------------ b. dead tiles on real data
DICT_ARMS = {"plain": None, "two_pow_103": np.float32(2.0 ** 103), "just_below": np.nextafter(np.float32(2.0 ** 103), np.float32(0)),
             "inf": np.float32(np.inf), "subnormal": np.float32(-(2.0 ** -140))}


@functools.lru_cache(maxsize=None)
def wide_coded(arm):
    """gen_wide's pattern (x spans ~77 column tiles) with 200 different real, mixed-sign weights (one-byte codes), one
    of them replaced by the arm's special value."""
    c = dict(data("wide"))
    rng = np.random.default_rng(71)
    pool = np.unique(F.wide_range(rng, 400))
    pool = pool[pool != 0][::2][:200]                     # (sorted: every other one, so that both signs are there)
    assert len(pool) == 200 and (pool < 0).any() and (pool > 0).any()
    if DICT_ARMS[arm] is not None:
        pool[3] = DICT_ARMS[arm]
    va = pool[rng.integers(0, 200, len(c["ci"]))]
    va[:200] = pool
    c["va"] = va.astype(np.float32)
    return c


@pytest.mark.parametrize("finite", [0, 1, 6, 2000])
@pytest.mark.parametrize("arm", list(DICT_ARMS))
def test_tiles_of_unreached_x_keep_the_oracles_bits(eng, plan, arm, finite):
    c = wide_coded(arm)
    rng = np.random.default_rng(72 + finite)
    x = np.where(rng.random(c["cols"]) < 0.5, FLT_MAX, -FLT_MAX).astype(np.float32)
    read = np.unique(c["ci"])
    at = rng.choice(read, finite, replace=False)            # columns that some row really reads
    if finite:
        at[0] = c["ci"][c["rp"][c["rows"] - 5]]             # ... one of them read by the 30 000-entry row
    vals = F.wide_range(rng, finite)
    if finite:
        vals[0] = -abs(vals[0]) - np.float32(1e-3)          # negative ones among them
    x[at] = vals
    assert finite == 0 or ((x[at] < 0).any() and finite - 1 <= (np.abs(x) < FLT_MAX).sum() <= finite)
    A = upload(eng, c, plan)
    if plan in ("tiled", "tiled-nofold", "tiled-8bit"):
        assert "values=dict8(" in A.describe(), A.describe()
    y = data("wide")["ys"][0]                                # real, with its own +-FLT_MAX entries
    for alpha, beta in M.EPILOGUES[:3]:
        want = O.kernel(MP, c["rp"], c["ci"], c["va"], x, y, alpha, beta, vlength=c["cols"])
        assert not np.isnan(want).any()
        got = run_spmv(eng, MP, A, c["rows"], x, y, alpha, beta)
        assert_bits(got, want, f"{arm}, {finite} reached x words, {plan}, alpha={alpha:g} beta={beta:g}")
    A.free()


# ------------------------------------------------------------------ c. sh_spmm
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", ["ragged", "clustered", "wide"])
def test_spmm_columns_equal_oracle_bit_for_bit(eng, name, width):
    c = data(name)
    if name == "ragged":
        deg = np.diff(c["rp"])
        assert {16, 17, 4096, 4097, 70001} <= set(deg.tolist())     # one-team limit, long-row threshold, several segments
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], plan=1)
    X, Y = interleave(c["xs"][:width], np.float32), interleave(c["ys"][:width], np.float32)
    for alpha, beta in M.EPILOGUES:
        got = run_spmm(eng, MP, A, c["rows"], X, Y, alpha, beta)
        for j in range(width):
            assert_bits(got[:, j], expected(name, j, alpha, beta), f"sh_spmm {name} width {width} column {j} alpha={alpha:g} beta={beta:g}")
    A.free()


# ------------------------------------------------------------------ d. the iteration loops
@functools.lru_cache(maxsize=None)
def coarse_delta(name):
    """The median size of the oracle's own vertex improvements from the first source: half of them fall below it."""
    rp, ci, va, n = M.graph(name)
    x0 = M.start_vector(n, M.sources(name)[0])
    _, it, _ = O.iterate(MP, rp, ci, va, x0, x0, 0.0, 0.0, EXACT, 5000)
    ch = M.launch_changes(lambda *a: O.kernel(MP, *a, 0.0, 0.0), rp, ci, va, x0, it)
    assert len(ch) > 1000
    return float(np.median(ch))


@functools.lru_cache(maxsize=None)
def oracle_run(name, source, delta):
    rp, ci, va, n = M.graph(name)
    x0 = M.start_vector(n, source)
    return O.iterate(MP, rp, ci, va, x0, x0, 0.0, 0.0, delta, 5000)


@functools.lru_cache(maxsize=None)
def float64_run(name, source):
    rp, ci, va, n = M.graph(name)
    return M.float64_sssp(rp, ci, va, source)


def deltas(name):
    return (EXACT, coarse_delta(name))


def run_iterate(eng, A, x0, delta, cap=5000, a=0.0, b=0.0):
    xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(len(x0)).fill(0)
    it, conv, _, _ = eng.iterate(MP, A, xv, yv, sc, a, b, delta=delta, max_iters=cap)
    got = xv.download(np.float32)
    for v in (xv, yv, sc):
        v.free()
    return got, it, conv


def run_frontier(eng, A, Fr, x0, delta, share, cap=5000, a=0.0, b=0.0):
    xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(len(x0)).fill(0)
    res = eng.iterate_frontier(MP, A, Fr, xv, yv, sc, a, b, delta=delta, max_iters=cap, dense_share=share)
    got = xv.download(np.float32)
    for v in (xv, yv, sc):
        v.free()
    return got, res


def run_multi(eng, A, starts, delta, cap=5000, a=0.0, b=0.0):
    n, width = len(starts[0]), len(starts)
    X0 = interleave(starts, np.float32)
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0)
    launches, iters, conv, _, _ = eng.iterate_multi(MP, A, xv, yv, sc, a, b, width, delta=delta, max_iters=cap)
    got = xv.download(np.float32, shape=(n, width))
    for v in (xv, yv, sc):
        v.free()
    return got, launches, iters, conv


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_the_coarse_delta_stops_the_oracle_early(name):
    """(What the second delta is for: many improvements fall below it, so the loop stops with bits still changing.)"""
    for source in M.sources(name)[:1]:
        full, coarse = oracle_run(name, source, EXACT), oracle_run(name, source, coarse_delta(name))
        assert full[2] and coarse[2] and coarse[1] < full[1] and (bits(full[0]) != bits(coarse[0])).any()


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_iterate_equals_oracle_and_meets_the_float64_bound(eng, plan, name):
    rp, ci, va, n = M.graph(name)
    A = eng.upload_csr(n, n, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    for source in M.sources(name):
        for delta in deltas(name):
            want, w_it, w_conv = oracle_run(name, source, delta)
            got, it, conv = run_iterate(eng, A, M.start_vector(n, source), delta)
            assert (it, conv) == (w_it, w_conv), f"{name} {plan} source {source} delta {delta:g}"
            assert_bits(got, want, f"sh_iterate {name} {plan} source {source} delta {delta:g}")
            if delta == EXACT:
                D, hops = float64_run(name, source)
                M.assert_within_path_bound(got, D, hops, it, what=f"sh_iterate {name} {plan} source {source}")
    A.free()


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_iterate_multi_width_8_equals_oracle_column_by_column(eng, name):
    rp, ci, va, n = M.graph(name)
    rng = np.random.default_rng(81)
    srcs = list(M.sources(name)) + [int(s) for s in rng.choice(np.arange(1, n - 1), 5, replace=False)]
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    for delta in deltas(name):
        ref = [oracle_run(name, s, delta) for s in srcs]
        got, launches, iters, conv = run_multi(eng, A, [M.start_vector(n, s) for s in srcs], delta)
        assert iters == [r[1] for r in ref] and conv == [r[2] for r in ref] and launches == max(iters), f"{name} delta {delta:g}"
        for j, s in enumerate(srcs):
            assert_bits(got[:, j], ref[j][0], f"sh_iterate_multi {name} source {s} (column {j}) delta {delta:g}")
            if delta == EXACT:
                D, hops = float64_run(name, s)
                M.assert_within_path_bound(got[:, j], D, hops, iters[j], what=f"sh_iterate_multi {name} source {s}")
    if name == "rmat15":
        assert len({r[1] for r in ref}) >= 2     # (columns freeze at different launches)
    A.free()


@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_iterate_frontier_equals_oracle_in_every_mode(eng, name, up):
    rp, ci, va, n = M.graph(name)
    A = eng.upload_csr(n, n, rp, ci, va, plan=up)
    Fr = eng.frontier(A, rp, ci, va)
    for source in M.sources(name):
        for delta in deltas(name):
            want, w_it, w_conv = oracle_run(name, source, delta)
            for share in (0.0, -1.0, 1.0):
                got, (it, conv, modes, changed, active, _, _) = run_frontier(eng, A, Fr, M.start_vector(n, source), delta, share)
                what = f"sh_iterate_frontier {name} plan {up} source {source} delta {delta:g} dense_share {share}"
                assert (it, conv) == (w_it, w_conv), what
                assert_bits(got, want, what)
                if share == 0.0:
                    assert not any(modes)
                elif delta == EXACT:
                    # thin wavefronts at the end of every run (and all through the grid) go sparse; the first two
                    # launches are always dense
                    print(f"[minplus] {what}: {sum(modes)} sparse and {len(modes) - sum(modes)} dense launches")
                    if share == 1.0 or name == "grid":     # (the default share is the grid's: its wavefronts are thin)
                        assert 1 in modes and 0 in modes, what
                if delta == EXACT and share != 0.0:
                    D, hops = float64_run(name, source)
                    M.assert_within_path_bound(got, D, hops, it, what=what)
    Fr.free()
    A.free()


@pytest.mark.parametrize("chunks", [1, 3])
def test_sharded_driver_equals_single_gpu_iterate(eng, chunks):
    """The in-process form of test_parity_gpu.py::test_sharded_driver_with_hip_local_step, on real weights."""
    import torch
    from sparseharness_amd.distributed import HipLocalStep, ShardedIteration, ShardPlan
    rp, ci, va, n = M.graph("rmat15")
    torch.cuda.set_device(0)
    sp = ShardPlan(rp, ci, va, 0, 1, chunks)
    A = eng.upload_csr(n, n, rp, ci, va)
    for source in M.sources("rmat15")[:2]:
        x0 = M.start_vector(n, source)
        for delta in deltas("rmat15"):
            want, w_it, w_conv = oracle_run("rmat15", source, delta)
            single, s_it, s_conv = run_iterate(eng, A, x0, delta)
            final, iters, conv = ShardedIteration(sp, MP, HipLocalStep(sp, MP, 0)).run(x0, x0, 0.0, 0.0, delta, 5000)
            assert (iters, conv) == (s_it, s_conv) == (w_it, w_conv), f"source {source} delta {delta:g}"
            assert_bits(final, single, f"sharded driver vs sh_iterate, source {source} delta {delta:g}")
            assert_bits(final, want, f"sharded driver vs the oracle, source {source} delta {delta:g}")
    A.free()


# ------------------------------------------------------------------ e. special values, one launch
INF, NAN = np.float32(np.inf), np.float32(np.nan)
SP_ROWS = len(special_pattern()[0]) - 1
SP_EPILOGUES = M.EPILOGUES + ((-(2.0 ** -140), 2.0 ** 127), (-0.0, -0.0))   # negative subnormal alpha, huge beta; minus zeros


def special_cases():
    """name -> (rp, ci, va, x, y, check(want) or None) on the hand-built pattern of tests/test_float_gpu.py: a short row,
    a 17..4096 row and a long row read column C1, three others C2, nobody else does."""
    rng = np.random.default_rng(91)
    rp, ci, at1, at2 = special_pattern()
    nnz = len(ci)
    pool = np.unique(F.wide_range(rng, 64))
    pool = pool[pool != 0][::3][:16]
    assert len(pool) == 16 and (pool < 0).any() and (pool > 0).any()
    va = pool[rng.integers(0, 16, nnz)].astype(np.float32)        # sixteen real values: a full four-bit table
    va[:16] = pool
    x = M.with_unreached(rng, F.wide_range(rng, SP_COLS))
    y = M.with_unreached(rng, F.wide_range(rng, SP_ROWS))
    hot = [R_SHORT, R_SHORT2, R_MID, R_LONG]
    out = {}

    def put(v, where, what):
        v = v.copy()
        v[where] = what
        return v

    def is_word(word, rows=slice(None)):
        return lambda want: (bits(want)[rows] == word).all()

    out["x_inf_and_minus_inf"] = (rp, ci, va, put(put(x, C1, INF), C2, -INF), y, None)
    out["y_inf"] = (rp, ci, va, x, put(put(y, hot, INF), [0, 5], -INF), None)
    out["weights_inf"] = (rp, ci, put(put(va, at1, INF), at2, -INF), x, y, None)
    # every product Inf and y Inf: the row is the identity seed -- FLT_MAX (+ |alpha|), not Inf
    signs = np.where(rng.random(SP_COLS) < 0.5, INF, -INF).astype(np.float32)
    out["every_x_inf_y_inf"] = (rp, ci, va, signs, np.full(SP_ROWS, INF, np.float32), "identity")
    out["every_weight_inf_y_inf"] = (rp, ci, np.where(va < 0, -INF, INF).astype(np.float32), x, np.full(SP_ROWS, -INF, np.float32), "identity")
    # rows whose entries are ALL outside [0, cols), every dictionary value >= 2^103 (so is whatever code 0 decodes to)
    big = (np.float32(2.0 ** 103) * np.arange(1, 17)).astype(np.float32) * np.where(np.arange(16) % 3 == 0, -1, 1).astype(np.float32)
    vbig = big[rng.integers(0, 16, nnz)]
    vbig[:16] = big
    stray = ci.copy()
    for r in hot:
        stray[rp[r]:rp[r + 1]] = np.where(rng.random(rp[r + 1] - rp[r]) < 0.5, -1 - rng.integers(0, 3, rp[r + 1] - rp[r]), SP_COLS + rng.integers(0, 99, rp[r + 1] - rp[r]))
    out["stray_rows_huge_dictionary"] = (rp, stray.astype(np.int32), vbig, x, put(y, hot, INF), ("identity", hot))
    # subnormals: k * 2^-149 + m * 2^-149 is exact and must not be flushed
    tiny = np.float32(2.0 ** -149)
    vsub = (rng.integers(1, 9, nnz) * rng.choice([-1, 1], nnz)).astype(np.float32) * tiny
    xsub = (rng.integers(1, 1000, SP_COLS) * rng.choice([-1, 1], SP_COLS)).astype(np.float32) * tiny
    ysub = (rng.integers(500, 1000, SP_ROWS)).astype(np.float32) * -tiny
    out["subnormal_weights_and_x"] = (rp, ci, vsub, xsub, ysub, "subnormal")
    mz = np.float32(-0.0)
    vz = np.where(rng.random(nnz) < 0.5, mz, np.float32(0.0)).astype(np.float32)
    out["minus_zero_everywhere"] = (rp, ci, vz, np.full(SP_COLS, mz, np.float32), np.full(SP_ROWS, mz, np.float32), "zero")
    out["minus_flt_max"] = (rp, ci, -np.abs(va), put(np.full(SP_COLS, -FLT_MAX, np.float32), [C1, 7, 1500], [-2.5, 1e-3, -7e4]),
                            put(np.full(SP_ROWS, -FLT_MAX, np.float32), [1, R_MID], [-3.25, 1e30]), None)
    return out


SPECIAL = special_cases()


def check_special(name, tag, want, alpha, beta):
    """What the oracle itself must say (so that the case tests what its name promises)."""
    assert not np.isnan(want).any(), name
    if tag is None:
        return
    rows = slice(None)
    if isinstance(tag, tuple):
        tag, rows = tag
    if tag == "identity":           # min(FLT_MAX + |alpha|, Inf)
        with np.errstate(over="ignore"):
            word = bits(np.float32(FLT_MAX) + np.abs(np.float32(alpha)))[0]
        assert (bits(want)[rows] == word).all(), name
        if abs(alpha) < 2.0 ** 100:
            assert word == 0x7F7FFFFF
    if tag == "zero" and alpha == 0 and beta == 0:
        assert (bits(want) == 0).all(), name
    if tag == "subnormal" and alpha == 0 and beta == 0:
        assert (want > 0).all() and (want < 2.0 ** -126).all(), name


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_values_spmv(eng, plan, name):
    rp, ci, va, x, y, tag = SPECIAL[name]
    A = eng.upload_csr(SP_ROWS, SP_COLS, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    for alpha, beta in SP_EPILOGUES:
        want = O.kernel(MP, rp, ci, va, x, y, alpha, beta, vlength=SP_COLS)
        check_special(name, tag, want, alpha, beta)
        got = run_spmv(eng, MP, A, SP_ROWS, x, y, alpha, beta)
        assert_bits(got, want, f"{name} {plan} alpha={alpha!r} beta={beta!r} [{A.describe()}]")
    A.free()


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_values_spmm_width_8(eng, name):
    """Columns 0 and 3 carry the special x / y; the others are real neighbours that must not notice."""
    rp, ci, va, x, y, tag = SPECIAL[name]
    rng = np.random.default_rng(92)
    xs = [x] + [M.with_unreached(rng, F.wide_range(rng, SP_COLS)) for _ in range(7)]
    ys = [y] + [M.with_unreached(rng, F.wide_range(rng, SP_ROWS)) for _ in range(7)]
    xs[3], ys[3] = x, y
    A = eng.upload_csr(SP_ROWS, SP_COLS, rp, ci, va, plan=1)
    for alpha, beta in SP_EPILOGUES:
        got = run_spmm(eng, MP, A, SP_ROWS, interleave(xs, np.float32), interleave(ys, np.float32), alpha, beta)
        for j in range(8):
            want = O.kernel(MP, rp, ci, va, xs[j], ys[j], alpha, beta, vlength=SP_COLS)
            assert_bits(got[:, j], want, f"{name} column {j} alpha={alpha!r} beta={beta!r}")
    A.free()


def test_special_values_on_the_ragged_matrix(eng, plan):
    """Inf, 2^103, subnormals, -0.0 and -FLT_MAX sprinkled over the weights, x and y of the ragged matrix (long rows, stray
    columns, the hub column): every row keeps the oracle's bits."""
    c = data("ragged")
    rng = np.random.default_rng(93)
    pick = np.array([INF, -INF, 2.0 ** 103, -(2.0 ** 110), 2.0 ** -149, -(2.0 ** -130), -0.0, 0.0, -FLT_MAX, FLT_MAX], np.float32)

    def sprinkle(v, share):
        v = v.copy()
        hit = rng.random(len(v)) < share
        v[hit] = pick[rng.integers(0, len(pick), int(hit.sum()))]
        return v

    va, x, y = sprinkle(c["va"], 0.05), sprinkle(c["x"], 0.1), sprinkle(c["y"], 0.1)
    x[1234] = INF                                              # the hub column
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    for alpha, beta in SP_EPILOGUES:
        want = O.kernel(MP, c["rp"], c["ci"], va, x, y, alpha, beta, vlength=c["cols"])
        assert not np.isnan(want).any()
        assert_bits(want, M.order_free(c["rp"], c["ci"], va, x, y, alpha, beta, c["cols"]), "the two references")
        got = run_spmv(eng, MP, A, c["rows"], x, y, alpha, beta)
        assert_bits(got, want, f"ragged with special values, {plan} alpha={alpha!r} beta={beta!r}")
    A.free()


# ------------------------------------------------------------------ e. NaN: rows that read none keep their bits
def nan_case():
    """M.nan_case on the ragged input set (the one tests/test_minplus_ref.py checks on the references)."""
    return M.nan_case(data("ragged"))


def test_rows_that_read_no_nan_keep_their_bits(eng, plan):
    rp, ci, va, x, y, exempt = nan_case()
    c = data("ragged")
    A = eng.upload_csr(c["rows"], c["cols"], rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    for alpha, beta in M.EPILOGUES[:3]:
        want = O.kernel(MP, rp, ci, va, x, y, alpha, beta, vlength=c["cols"])
        assert not np.isnan(want[~exempt]).any()
        got = run_spmv(eng, MP, A, c["rows"], x, y, alpha, beta)
        assert_bits(got[~exempt], want[~exempt], f"rows that read no NaN, {plan} alpha={alpha:g} beta={beta:g}")
    A.free()
    # a NaN in x that no entry points at, on the hand-built pattern: no row is exempt
    rp2, ci2, _, _ = special_pattern(referenced=False)
    _, _, va2, x2, y2, _ = SPECIAL["x_inf_and_minus_inf"]
    x2 = x2.copy()
    x2[C1] = NAN
    assert not M.rows_reading_nan(rp2, ci2, va2, x2, y2, SP_COLS).any()
    A = eng.upload_csr(SP_ROWS, SP_COLS, rp2, ci2, va2)
    got = run_spmv(eng, MP, A, SP_ROWS, x2, y2, 0.25, 1.5)
    assert_bits(got, O.kernel(MP, rp2, ci2, va2, x2, y2, 0.25, 1.5, vlength=SP_COLS), f"a NaN nobody reads, {plan}")
    A.free()


def test_rows_that_read_no_nan_keep_their_bits_in_spmm(eng):
    rp, ci, va, x, y, exempt = nan_case()
    c = data("ragged")
    A = eng.upload_csr(c["rows"], c["cols"], rp, ci, va, plan=1)
    xs, ys = [x] + c["xs"][:7], [y] + c["ys"][:7]
    got = run_spmm(eng, MP, A, c["rows"], interleave(xs, np.float32), interleave(ys, np.float32), 0.25, 1.5)
    for j in range(8):
        ex = M.rows_reading_nan(rp, ci, va, xs[j], ys[j], c["cols"])
        assert ex.sum() < 0.01 * c["rows"]
        want = O.kernel(MP, rp, ci, va, xs[j], ys[j], 0.25, 1.5, vlength=c["cols"])
        assert_bits(got[~ex, j], want[~ex], f"column {j}")
    A.free()


# ------------------------------------------------------------------ e. special values in the iteration loops
def special_graph(n=2000, seed=95):
    """A square graph for the loops: rows of 0..12 entries, row 700 with 9000 entries whose weights are ALL +-Inf, row 1400
    with 5000 real ones (both above the long-row threshold: cut into pieces by every kernel), real weights with Inf, 2^103,
    subnormals and -0.0 among them, stray columns."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 13, n).astype(np.int64)
    deg[700], deg[1400] = 9000, 5000
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, n, nnz).astype(np.int32)
    ci[rng.random(nnz) < 0.02] = n + 3
    va = M.real_weights(rng, nnz)
    pick = np.array([INF, -INF, 2.0 ** 103, 2.0 ** -149, -(2.0 ** -140), -0.0], np.float32)
    hit = rng.random(nnz) < 0.1
    va[hit] = pick[rng.integers(0, len(pick), int(hit.sum()))]
    va[rp[700]:rp[701]] = np.where(rng.random(9000) < 0.5, INF, -INF)
    return rp, ci, va, n


def special_start(n, source):
    x0 = np.full(n, FLT_MAX, np.float32)
    x0[1::7] = -FLT_MAX
    x0[source] = -0.0
    x0[(source + 11) % n] = np.float32(2.0 ** -145)
    return x0


# (alpha, beta, launch cap): the app's scalars; a negative subnormal alpha with a huge beta -- |x[r]| + 2^103 is Inf for an
# unreached vertex, so a row whose products are all Inf shows whether its minimum started from the identity
LOOP_SCALARS = ((0.0, 0.0, 200), (-(2.0 ** -140), 2.0 ** 103, 12))


@functools.lru_cache(maxsize=None)
def special_oracle(source, which):
    rp, ci, va, n = special_graph()
    a, b, cap = LOOP_SCALARS[which]
    x0 = special_start(n, source)
    want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, a, b, EXACT, cap)
    assert not np.isnan(want).any() and not np.isinf(want).any()
    if which == 1:
        assert bits(want)[700] == 0x7F7FFFFF      # the all-Inf row: the identity, although |x[r]| + beta is Inf
    return want, it, conv


@pytest.mark.parametrize("which", [0, 1])
def test_special_values_in_iterate(eng, plan, which):
    rp, ci, va, n = special_graph()
    a, b, cap = LOOP_SCALARS[which]
    A = eng.upload_csr(n, n, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    for source in (0, 1999):
        want, w_it, w_conv = special_oracle(source, which)
        got, it, conv = run_iterate(eng, A, special_start(n, source), EXACT, cap, a, b)
        assert (it, conv) == (w_it, w_conv)
        assert_bits(got, want, f"sh_iterate special graph {plan} source {source} scalars {which}")
    A.free()


@pytest.mark.parametrize("which", [0, 1])
def test_special_values_in_iterate_multi_and_frontier(eng, which):
    rp, ci, va, n = special_graph()
    a, b, cap = LOOP_SCALARS[which]
    srcs = (0, 1999, 5, 1000)
    ref = [special_oracle(s, which) for s in srcs]
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    got, launches, iters, conv = run_multi(eng, A, [special_start(n, s) for s in srcs], EXACT, cap, a, b)
    assert iters == [r[1] for r in ref] and conv == [r[2] for r in ref]
    for j, s in enumerate(srcs):
        assert_bits(got[:, j], ref[j][0], f"sh_iterate_multi special graph source {s} scalars {which}")
    Fr = eng.frontier(A, rp, ci, va)
    for j, s in enumerate(srcs[:2]):
        for share in (0.0, -1.0, 1.0):
            got, res = run_frontier(eng, A, Fr, special_start(n, s), EXACT, share, cap, a, b)
            assert res[:2] == ref[j][1:], (s, share)
            assert_bits(got, ref[j][0], f"sh_iterate_frontier special graph source {s} dense_share {share} scalars {which}")
            if share == 1.0:
                assert 1 in res[2]               # (the long rows were pulled by sparse launches too)
    Fr.free()
    A.free()


@pytest.mark.parametrize("chunks", [1, 3])
def test_special_values_in_the_sharded_driver(chunks):
    import torch
    from sparseharness_amd.distributed import HipLocalStep, ShardedIteration, ShardPlan
    rp, ci, va, n = special_graph()
    torch.cuda.set_device(0)
    sp = ShardPlan(rp, ci, va, 0, 1, chunks)
    for which, (a, b, cap) in enumerate(LOOP_SCALARS):
        want, w_it, w_conv = special_oracle(0, which)
        x0 = special_start(n, 0)
        final, iters, conv = ShardedIteration(sp, MP, HipLocalStep(sp, MP, 0)).run(x0, x0, a, b, EXACT, cap)
        assert (iters, conv) == (w_it, w_conv)
        assert_bits(final, want, f"sharded driver, special graph, chunks {chunks} scalars {which}")


# ------------------------------------------------------------------ e. an Inf in x0
def inf_start_case():
    """With alpha = 0 an Inf vertex is replaced by min(dot, Inf) <= FLT_MAX at once: one launch sees |Inf - FLT_MAX| = Inf,
    then the loop goes on as usual.  With alpha = Inf every row keeps |x[r]| + |beta|: the Inf stays, |Inf - Inf| is NaN,
    `differs` stays true and the loop runs to its cap unconverged."""
    rp, ci, va, n = M.weighted_grid(12, 20, seed=96)
    x0 = M.start_vector(n, 3)
    x0[57] = INF
    return rp, ci, va, n, x0


INF_SCALARS = ((0.0, 0.0), (np.inf, 0.0))
INF_CAP = 9


def test_the_oracle_on_an_inf_start():
    rp, ci, va, n, x0 = inf_start_case()
    want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, np.inf, 0.0, EXACT, INF_CAP)
    assert (it, conv) == (INF_CAP, False) and np.isinf(want[57]) and (bits(want) == bits(np.abs(x0))).all()
    want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, 0.0, 0.0, EXACT, INF_CAP)
    assert (it, conv) == (INF_CAP, False) and np.isfinite(want).all()     # (the 30-hop grid needs more than 9 launches)


@pytest.mark.parametrize("a,b", INF_SCALARS)
def test_an_inf_start_runs_like_the_oracle(eng, plan, a, b):
    rp, ci, va, n, x0 = inf_start_case()
    want, w_it, w_conv = O.iterate(MP, rp, ci, va, x0, x0, a, b, EXACT, INF_CAP)
    A = eng.upload_csr(n, n, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    got, it, conv = run_iterate(eng, A, x0, EXACT, INF_CAP, a, b)
    assert (it, conv) == (w_it, w_conv)
    assert_bits(got, want, f"sh_iterate from an Inf, {plan} alpha={a}")
    # sh_iterate_frontier is held to the oracle where the Inf does not persist (alpha = 0).  Where it does (alpha = Inf) the
    # word is outside its contract (include/sparseharness_hip.h): a row that is not recomputed must pass |in - out| < delta,
    # and |Inf - Inf| is NaN.  What the loop does there is pinned: dense launches raise `differs` as sh_iterate's do, so
    # dense_share = 0 runs to the cap like the oracle; no word's bits change, so the first sparse launch (launch 2) has
    # nothing to recompute and reports converged.  The vector is the oracle's in every mode.
    if plan in ("stream", "tiled"):
        Fr = eng.frontier(A, rp, ci, va)
        for share in (0.0, -1.0, 1.0):
            got, res = run_frontier(eng, A, Fr, x0, EXACT, share, INF_CAP, a, b)
            what = f"sh_iterate_frontier from an Inf, {plan} alpha={a} dense_share {share}"
            if np.isfinite(a) or share == 0.0:
                assert res[:2] == (w_it, w_conv), what
            else:
                assert res[:2] == (3, True) and res[2] == [0, 0, 1] and res[3] == [0, 0, 0] and res[4][2] == 0, (what, res[:5])
            assert_bits(got, want, what)
        Fr.free()
    if plan == "stream":
        clean = M.start_vector(n, 3)
        c_want, c_it, c_conv = O.iterate(MP, rp, ci, va, clean, clean, a, b, EXACT, INF_CAP)
        got, launches, iters, conv = run_multi(eng, A, [clean, x0, clean, x0], EXACT, INF_CAP, a, b)
        assert iters == [c_it, w_it, c_it, w_it] and conv == [c_conv, w_conv, c_conv, w_conv]
        for j in range(4):
            assert_bits(got[:, j], c_want if j % 2 == 0 else want, f"sh_iterate_multi column {j} alpha={a}")
    A.free()


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("a,b", INF_SCALARS)
def test_an_inf_start_in_the_sharded_driver(a, b, chunks):
    """The driver's changed flag is `differs` over every row of every launch, as sh_iterate's: a persisting Inf keeps it
    raised to the cap."""
    import torch
    from sparseharness_amd.distributed import HipLocalStep, ShardedIteration, ShardPlan
    rp, ci, va, n, x0 = inf_start_case()
    want, w_it, w_conv = O.iterate(MP, rp, ci, va, x0, x0, a, b, EXACT, INF_CAP)
    assert (w_it, w_conv) == (INF_CAP, False)
    torch.cuda.set_device(0)
    sp = ShardPlan(rp, ci, va, 0, 1, chunks)
    final, iters, conv = ShardedIteration(sp, MP, HipLocalStep(sp, MP, 0)).run(x0, x0, a, b, EXACT, INF_CAP)
    assert (iters, conv) == (w_it, w_conv)
    assert_bits(final, want, f"sharded driver from an Inf, chunks {chunks} alpha={a}")
