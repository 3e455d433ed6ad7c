"""(+,x) on real floats, on the GPU: sh_spmv under the five plan variants, sh_spmm and sh_iterate_multi on the CSR-stream
plan at widths 4..32.

  a. accuracy: every row within float_ref.bound() of the float64 result (a derived worst case for any summation order,
     see tests/float_ref.py; tests/test_float_bound.py shows that the sequential float32 oracle meets it on the same
     inputs and that 16-bit values or x do not),
  b. structure of sh_spmm (+,x): integer-valued data bit for bit against the oracle and sh_spmv through the long-row
     segments and their fix-up; one-team rows on general floats bit for bit,
  c. sh_iterate_multi (+,x) with columns that freeze at different launches across the fix-up,
  d. +-Inf, NaN, subnormals and signed zeros in x, y and the values: bit for bit against the oracle (the finite part
     of the data is small integers, so every order gives the same result), a NaN for a NaN.
No tolerance here comes from the device's output.
"""
import functools
import re

import numpy as np
import pytest

import float_ref as F
from oracle import oracle as O
from sparseharness_amd.engine import Engine
from test_multi_gpu import bits, interleave, ragged_csr, run_spmm, run_spmv
from test_parity_gpu import clustered_matrix

pytestmark = pytest.mark.gpu

PT = O.PLUS_TIMES_F32
WIDTHS = [4, 8, 16, 32]
PLANS = ["stream", "tiled", "tiled-8bit", "tiled-raw", "tiled-nofold"]


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


GENERATORS = {
    "ragged": F.gen_ragged,
    "clustered": functools.partial(F.gen_clustered, clustered_matrix),
    "wide": F.gen_wide,
    "few16": functools.partial(F.gen_few_values, 16),
    "few255": functools.partial(F.gen_few_values, 255),
    "few4000": functools.partial(F.gen_few_values, 4000),
}
# values=... of describe() per few-values input and plan variant (plan_common.h, decide_value_coding)
CODING = {("few16", "tiled"): "dict4(16)", ("few16", "tiled-nofold"): "dict4(16)", ("few16", "tiled-8bit"): "dict8(17)",
          ("few255", "tiled"): "dict8(256)", ("few255", "tiled-nofold"): "dict8(256)", ("few255", "tiled-8bit"): "dict8(256)",
          ("few4000", "tiled"): "dict16(4001)", ("few4000", "tiled-nofold"): "dict16(4001)", ("few4000", "tiled-8bit"): "raw",
          ("few16", "tiled-raw"): "raw", ("few255", "tiled-raw"): "raw", ("few4000", "tiled-raw"): "raw"}


@functools.lru_cache(maxsize=None)
def data(name):
    """The input set `name` with 32 further x / y columns and the float64 rows of x (those of a column: exact_of)."""
    c = GENERATORS[name](width=32)
    c["name"] = name
    c["exact"] = F.exact_rows(c["rp"], c["ci"], c["va"], c["x"], c["cols"])
    c["exact_cols"] = {}
    return c


def exact_of(c, j):
    if j not in c["exact_cols"]:
        c["exact_cols"][j] = F.exact_rows(c["rp"], c["ci"], c["va"], c["xs"][j], c["cols"])
    return c["exact_cols"][j]


# ------------------------------------------------------------------ a. accuracy against float64
@pytest.mark.parametrize("name", list(GENERATORS))
def test_spmv_rows_within_float32_bound(eng, plan, name):
    c = data(name)
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"])
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    if (name, plan) in CODING:
        assert f"values={CODING[(name, plan)]}" in A.describe(), A.describe()
    if name == "clustered" and plan.startswith("tiled"):
        assert (" folded" in A.describe()) == (plan != "tiled-nofold"), A.describe()
    if name == "wide" and plan.startswith("tiled"):
        assert int(re.search(r"tiles=(\d+)", A.describe()).group(1)) > 50, A.describe()
    dot, mag, n = c["exact"]
    for alpha, beta, with_y in F.EPILOGUES:
        y = c["y"] if with_y else None
        got = run_spmv(eng, PT, A, c["rows"], c["x"], y, alpha, beta)
        F.assert_within(got, dot, mag, n, alpha, y, beta, what=f"sh_spmv {name} {plan} alpha={alpha:g} beta={beta:g}")
    A.free()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", list(GENERATORS))
def test_spmm_columns_within_float32_bound(eng, name, width):
    """Every column of sh_spmm, and sh_spmv on that column through the same device matrix, within the bound."""
    c = data(name)
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], plan=1)
    X = interleave(c["xs"][:width], np.float32)
    for alpha, beta, with_y in F.EPILOGUES:
        Y = interleave(c["ys"][:width], np.float32) if with_y else None
        got = run_spmm(eng, PT, A, c["rows"], X, Y, alpha, beta)
        worst = 0.0
        for j in range(width):
            dot, mag, n = exact_of(c, j)
            y = c["ys"][j] if with_y else None
            what = f"{name} width {width} column {j} alpha={alpha:g} beta={beta:g}"
            worst = max(worst, F.assert_within(got[:, j], dot, mag, n, alpha, y, beta, what="sh_spmm " + what))
            if j % 4 == 1 or width == 4:   # (the single-vector path: every column at width 4, every fourth one above)
                single = run_spmv(eng, PT, A, c["rows"], c["xs"][j], y, alpha, beta)
                F.assert_within(single, dot, mag, n, alpha, y, beta, what="sh_spmv on " + what)
        print(f"[float bound] sh_spmm {name} width {width} alpha={alpha:g}: worst err/bound over the columns {worst:.3f}")
    A.free()


# ------------------------------------------------------------------ b. sh_spmm (+,x) structure, bit for bit
def integer_case(which):
    if which == "multi_gpu_ragged":
        rows, cols = 3001, 2500
        rp, ci, rng = ragged_csr(100 + PT, rows, cols, long_len=20_001)   # three segments and the fix-up
    else:
        rows, cols = F.RAGGED_ROWS, F.RAGGED_COLS
        rp, ci, rng = F.ragged_pattern()
    va = rng.integers(1, 17, rp[-1]) * rng.choice([-1, 1], rp[-1])        # |row sum| <= 70 001 * 16 * 3 < 2^24: exact
    xs = [rng.integers(-3, 4, cols).astype(np.float32) for _ in range(32)]
    ys = [rng.integers(-50, 51, rows).astype(np.float32) for _ in range(32)]
    return rows, cols, rp, ci, va.astype(np.float32), xs, ys


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("which", ["multi_gpu_ragged", "float_ragged"])
def test_spmm_plus_times_column_equals_single_vector_path_and_oracle(eng, which, width):
    """The (+,x) row of test_multi_gpu.py::test_column_equals_single_vector_path_and_oracle: long-row segments,
    spmm_long_fixup, wave-summed rows with stray columns, the alpha / beta / Y epilogue."""
    rows, cols, rp, ci, va, xs, ys = integer_case(which)
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    got = run_spmm(eng, PT, A, rows, interleave(xs[:width], np.float32), interleave(ys[:width], np.float32), 2.0, 0.5)
    for j in range(width):
        want = O.kernel(PT, rp, ci, va, xs[j], ys[j], 2.0, 0.5, vlength=cols)
        np.testing.assert_array_equal(bits(got[:, j]), bits(want), err_msg=f"column {j} vs the oracle")
        single = run_spmv(eng, PT, A, rows, xs[j], ys[j], 2.0, 0.5)
        np.testing.assert_array_equal(bits(got[:, j]), bits(single), err_msg=f"column {j} vs sh_spmv")
    A.free()


def stored_order_kernel(rp, ci, va, x, y, alpha, beta, cols):
    """O.kernel sums a row from its LAST stored entry to its first (the Lift kernels' reduce over the reversed row:
    oracle/sh_oracle.c, "the row is reduced in REVERSE stored order").  Handing it every row's entries back to front
    gives the sequential float32 sum in stored order -- Gold<float>::spmv's order -- through the same epilogue."""
    pos = np.arange(len(ci), dtype=np.int64)
    row_of = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    rev = rp[row_of].astype(np.int64) + rp[row_of + 1] - 1 - pos
    return O.kernel(PT, rp, ci[rev], va[rev], x, y, alpha, beta, vlength=cols)


@pytest.mark.parametrize("width", WIDTHS)
def test_spmm_one_team_rows_equal_sequential_float32_bit_for_bit(eng, width):
    """multi.hip.h:12: "rows of <= MM_SHORT entries are summed by ONE team, sequentially in stored order", with mul and
    add kept apart -- so on GENERAL floats those rows equal a sequential float32 loop bit for bit.  The loop is O.kernel.
    Stored order is a documented difference from O.kernel's own (reverse) order: rows of up to two entries, where the
    two orders coincide, are compared with O.kernel as it stands, longer ones with O.kernel run over the rows stored
    back to front (stored_order_kernel).  -0.0 + 0.0 seeds, stray columns and the y epilogue included."""
    c = data("ragged")
    deg = np.diff(c["rp"])
    short = deg <= 16                      # MM_SHORT: all stored entries count, stray columns too
    assert short.sum() > 1000 and (deg[short] == 16).any() and (deg == 17).any() and (deg[short] >= 3).sum() > 500
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], plan=1)
    for alpha, beta, with_y in F.EPILOGUES[:2]:
        Y = interleave(c["ys"][:width], np.float32) if with_y else None
        got = run_spmm(eng, PT, A, c["rows"], interleave(c["xs"][:width], np.float32), Y, alpha, beta)
        for j in range(width):
            y = c["ys"][j] if with_y else np.zeros(c["rows"], np.float32)
            want = stored_order_kernel(c["rp"], c["ci"], c["va"], c["xs"][j], y, alpha, beta, c["cols"])
            np.testing.assert_array_equal(bits(got[short, j]), bits(want[short]), err_msg=f"column {j}, alpha {alpha}")
            as_is = O.kernel(PT, c["rp"], c["ci"], c["va"], c["xs"][j], y, alpha, beta, vlength=c["cols"])
            np.testing.assert_array_equal(bits(got[deg <= 2, j]), bits(as_is[deg <= 2]), err_msg=f"column {j}, alpha {alpha}, O.kernel as it stands")
    A.free()


# ------------------------------------------------------------------ c. sh_iterate_multi (+,x) across the fix-up
def damped_stochastic(n=25_000, long_len=20_001, seed=21):
    """0.85 * a column-stochastic matrix: column c spreads x[c] evenly over its 1..8 target rows; row n // 3 is a
    target of `long_len` different columns (three long-row segments and the fix-up).  -> CSR by rows."""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 9, n)
    col = np.repeat(np.arange(n, dtype=np.int64), k)
    row = rng.integers(0, n, len(col))
    hub = rng.choice(n, long_len, replace=False)
    col, row = np.concatenate([col, hub]), np.concatenate([row, np.full(long_len, n // 3)])
    outdeg = np.bincount(col, minlength=n)
    val = (0.85 / outdeg[col]).astype(np.float32)
    order = np.lexsort((col, row))
    rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int32)
    return rp, col[order].astype(np.int32), val[order], n


def float64_iterates(rp, ci, va, x0, beta, launches):
    """x_k = A x_(k-1) + beta * x_(k-1) in float64 for k = 1..launches, with a running bound E_k on what ANY float32
    evaluation can be off by after k launches (the bound of float_ref applied per launch): the device holds xh with
    |xh - x| <= E, one launch on xh is off by at most bound(n, |A| |xh|, 1, xh, beta) <= bound(n, |A| (|x| + E), 1, |x| + E, beta),
    and the exact launch carries E on as |A| E + |beta| E.  -> {k: (x_k, E_k)}"""
    n = len(rp) - 1
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    a, b = va.astype(np.float64), F.f32(beta)
    cnt = np.diff(rp).astype(np.float64)
    x, E, out = x0.astype(np.float64), np.zeros(n), {}
    for k in range(1, launches + 1):
        reach = np.abs(x) + E
        mag = np.bincount(row_of, weights=np.abs(a) * reach[ci], minlength=n)
        E = np.bincount(row_of, weights=np.abs(a) * E[ci], minlength=n) + abs(b) * E + F.bound(cnt, mag, 1.0, reach, beta)
        x = np.bincount(row_of, weights=a * x[ci], minlength=n) + b * x
        out[k] = (x, E)
    return out


def test_iterate_multi_plus_times_columns_freeze_across_the_fixup(eng):
    """Four start vectors whose single sh_iterate runs stop at four different launch counts: in sh_iterate_multi every
    column stops at its own count, frozen columns are carried through the stream blocks AND spmm_long_fixup, and the
    vectors stay within the per-launch bound (float64_iterates: the bound of float_ref applied at every launch and
    carried forward, not gamma * iters) of the float64 iteration."""
    rp, ci, va, n = damped_stochastic()
    assert np.diff(rp).max() == np.diff(rp)[n // 3] >= 20_001
    width = 4
    rng = np.random.default_rng(22)
    beta = np.float32(0.15) / np.float32(n)
    starts = [(s * rng.uniform(0.5, 1.5, n)).astype(np.float32) for s in (1e-2, 1.0, 1e2, 1e4)]
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    single = []
    for x0 in starts:
        xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
        it, conv, _, _ = eng.iterate(PT, A, xv, yv, sc, 1.0, beta, delta=1e-4, max_iters=2000)
        single.append((xv.download(np.float32), it, conv))
        for v in (xv, yv, sc):
            v.free()
    print("[float bound] launches of the four single runs:", [s[1] for s in single])
    assert len({s[1] for s in single}) == 4 and all(s[2] for s in single)
    X0 = interleave(starts, np.float32)
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0)
    launches, iters, conv, _, _ = eng.iterate_multi(PT, A, xv, yv, sc, 1.0, beta, width, delta=1e-4, max_iters=2000)
    got = xv.download(np.float32, shape=(n, width))
    for v in (xv, yv, sc):
        v.free()
    A.free()
    assert iters == [s[1] for s in single] and conv == [s[2] for s in single] and launches == max(iters)
    for j in range(width):
        x, E = float64_iterates(rp, ci, va, starts[j], beta, iters[j])[iters[j]]
        for who, vec in (("sh_iterate_multi", got[:, j]), ("sh_iterate", single[j][0])):
            r = np.abs(vec.astype(np.float64) - x) / E
            r = np.where(np.isfinite(r), r, np.inf)
            print(f"[float bound] {who} column {j} after {iters[j]} launches: worst err/bound {r.max():.2e} at row {int(np.argmax(r))}")
            assert not (r > 1.0).any(), f"{who} column {j}: {(r > 1.0).sum()} rows outside, worst {r.max():.3f} at row {int(np.argmax(r))}"


# ------------------------------------------------------------------ d. special values
SP_COLS = 3000
C1, C2 = 0, SP_COLS - 1          # the special columns: the first and the last of x
SP_LENGTHS = [0, 1, 3, 16, 16, 17, 100, 1000, 4096, 20_001, 5, 0, 40, 300]
R_SHORT, R_SHORT2, R_MID, R_LONG = 2, 3, 6, 9


def special_pattern(referenced=True, seed=31):
    """A short row, a 17..4096 row and a heavy / long row reference column C1 once each (none does when `referenced`
    is False); the 17..4096 row and the long row also reference C2, as does one short row of its own.  No other entry
    points at C1 or C2; some columns lie outside [0, cols).  -> (rp, ci, positions of the C1 entries, of the C2 entries)"""
    rng = np.random.default_rng(seed)
    deg = np.array(SP_LENGTHS + rng.integers(1, 30, 60).tolist(), np.int64)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = (1 + rng.integers(0, SP_COLS - 2, nnz)).astype(np.int32)      # 1 .. cols - 2
    stray = rng.random(nnz) < 0.01
    ci[stray] = np.where(rng.random(int(stray.sum())) < 0.5, -1, SP_COLS + 7)
    at1 = np.array([rp[R_SHORT] + 1, rp[R_MID] + 50, rp[R_LONG] + 12_345], np.int64)
    at2 = np.array([rp[R_SHORT2] + 15, rp[R_MID] + 51, rp[R_LONG] + 99], np.int64)
    if referenced:
        ci[at1] = C1
    ci[at2] = C2
    return rp, ci, at1, at2


def small_ints(rng, n, lo=-3, hi=4):
    return rng.integers(lo, hi, n).astype(np.float32)


def special_cases():
    """name -> (referenced, va, x, [(alpha, beta, y)], value coding under the default policy or None)"""
    rng = np.random.default_rng(32)
    rows = len(SP_LENGTHS) + 60
    rp, ci, at1, at2 = special_pattern()
    nnz = len(ci)
    w16 = np.concatenate([np.arange(1, 9), -np.arange(1, 9)]).astype(np.float32)     # a full four-bit table
    va = w16[rng.integers(0, 16, nnz)]
    va[:16] = w16
    x = small_ints(rng, SP_COLS)
    y = small_ints(rng, rows, -50, 51)
    plain = [(1.0, 0.0, None), (-2.0, 0.5, y)]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    out = {}

    def put(v, where, what):
        v = v.copy()
        v[where] = what
        return v

    out["x_inf"] = (True, va, put(x, C1, inf), plain, "dict4(16)")
    xi = put(put(x, C1, inf), C2, -inf)
    out["x_inf_and_minus_inf"] = (True, put(put(va, at1, 1.0), at2, 1.0), xi, plain, "dict4(16)")
    out["x_nan"] = (True, va, put(x, C1, nan), plain, "dict4(16)")
    out["x_nan_referenced_by_nobody"] = (False, va, put(x, C1, nan), plain, "dict4(16)")
    out["stored_zero_times_inf"] = (True, put(va, at1, 0.0), put(x, C1, inf), plain, "dict8(17)")
    v15 = np.where(va == -8.0, np.float32(7.0), va)       # 15 finite values + Inf: 16 words that may NOT borrow code 0
    out["stored_inf_times_zero"] = (True, put(v15, at1, inf), put(x, C1, 0.0), plain, "dict8(17)")
    out["stored_inf_times_one"] = (True, put(v15, at1, inf), put(x, C1, 1.0), plain, "dict8(17)")
    tiny = np.float32(2.0 ** -140)
    out["x_subnormal"] = (True, va, x * tiny, [(1.0, 0.0, None), (-2.0, 0.5, y * np.float32(2.0 ** -139))], "dict4(16)")
    half = np.float32(2.0 ** -70)                        # normal factors, subnormal products: k * w * 2^-140
    out["products_subnormal"] = (True, va * half, x * half, [(1.0, 0.0, None), (-2.0, 0.5, y * np.float32(2.0 ** -139))], "dict4(16)")
    mz = np.full(rows, -0.0, np.float32)
    ymix = np.where(rng.random(rows) < 0.5, np.float32(-0.0), y).astype(np.float32)
    zeros = [(1.0, 0.0, None), (-2.0, 0.0, None), (2.0, 0.5, mz), (-2.0, 0.5, mz), (-2.0, 0.5, ymix), (1.0, 1.0, ymix)]
    neg = -np.abs(va)
    neg[:16] = -np.arange(1, 17)                         # sixteen negative weights: a full table again
    out["all_gathered_x_zero_negative_weights"] = (True, neg.astype(np.float32), np.zeros(SP_COLS, np.float32), zeros, "dict4(16)")
    out["x_minus_zero_everywhere"] = (True, va, np.full(SP_COLS, -0.0, np.float32), zeros, "dict4(16)")
    xz = np.where(rng.random(SP_COLS) < 0.7, np.float32(0.0), x).astype(np.float32)   # most rows of <= 16 entries gather zeros only
    out["mostly_zero_x_negative_weights"] = (True, neg.astype(np.float32), xz, zeros, "dict4(16)")
    return out


SPECIAL = special_cases()


def assert_same_or_nan(got, want, msg):
    """Bit for bit, except that a NaN of the oracle is matched by any NaN."""
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{msg}: rows {np.nonzero(nan & ~np.isnan(got))[0][:8]} should be NaN, got {got[nan & ~np.isnan(got)][:8]}"
    bad = np.nonzero(bits(got) != bits(want))[0]
    bad = bad[~nan[bad]]
    assert len(bad) == 0, f"{msg}: rows {bad[:8]} got {got[bad[:8]]!r} ({bits(got)[bad[:8]]}) want {want[bad[:8]]!r} ({bits(want)[bad[:8]]})"


def special_expectation(name, x, y, alpha, beta):
    referenced, va, _, _, _ = SPECIAL[name]
    rp, ci, at1, at2 = special_pattern(referenced)
    rows = len(rp) - 1
    yy = np.zeros(rows, np.float32) if y is None else y
    want = O.kernel(PT, rp, ci, va, x, yy, alpha, beta, vlength=SP_COLS)
    # rows that do not reference a special column: what the all-finite x gives (x[C1], x[C2] as any small integer)
    calm = x.copy()
    calm[[C1, C2]] = 1.0
    untouched = np.ones(rows, bool)
    untouched[[R_SHORT2, R_MID, R_LONG] + ([R_SHORT] if referenced else [])] = False
    calm_out = O.kernel(PT, rp, ci, va, calm, yy, alpha, beta, vlength=SP_COLS)
    assert np.array_equal(bits(want[untouched]), bits(calm_out[untouched]))
    if name.startswith(("x_inf", "x_nan")) and referenced:
        assert not np.isfinite(want[[R_SHORT, R_MID, R_LONG]]).any()
    if name == "x_inf_and_minus_inf":
        assert np.isnan(want[[R_MID, R_LONG]]).all() and np.isinf(want[[R_SHORT, R_SHORT2]]).all()
    if name in ("stored_zero_times_inf", "stored_inf_times_zero"):
        assert np.isnan(want[[R_SHORT, R_MID, R_LONG]]).all()
    return rp, ci, va, want, untouched, calm_out


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_values_spmv(eng, plan, name):
    referenced, va, x, epilogues, coding = SPECIAL[name]
    rp, ci, _, _ = special_pattern(referenced)
    rows = len(rp) - 1
    A = eng.upload_csr(rows, SP_COLS, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0], A.describe()
    if plan in ("tiled", "tiled-nofold"):
        assert f"values={coding}" in A.describe(), A.describe()
    for alpha, beta, y in epilogues:
        _, _, _, want, untouched, calm_out = special_expectation(name, x, y, alpha, beta)
        got = run_spmv(eng, PT, A, rows, x, y, alpha, beta)
        assert_same_or_nan(got, want, f"{name} {plan} alpha={alpha} beta={beta}")
        np.testing.assert_array_equal(bits(got[untouched]), bits(calm_out[untouched]), err_msg="rows that do not reference the special columns")
    A.free()


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_values_spmm_width_8(eng, name):
    """Column 0 carries the special x; the other seven are finite neighbours that must not notice."""
    referenced, va, x, epilogues, _ = SPECIAL[name]
    rp, ci, _, _ = special_pattern(referenced)
    rows = len(rp) - 1
    rng = np.random.default_rng(33)
    xs = [x, small_ints(rng, SP_COLS)] + [np.roll(x, 1 + j) if j % 2 else small_ints(rng, SP_COLS) for j in range(6)]
    xs[3] = x                                                   # (and the special x once more, in the lane's last word)
    A = eng.upload_csr(rows, SP_COLS, rp, ci, va, plan=1)
    for alpha, beta, y in epilogues:
        Y = None if y is None else interleave([y] * 8, np.float32)
        got = run_spmm(eng, PT, A, rows, interleave(xs, np.float32), Y, alpha, beta)
        for j in range(8):
            yy = np.zeros(rows, np.float32) if y is None else y
            want = O.kernel(PT, rp, ci, va, xs[j], yy, alpha, beta, vlength=SP_COLS)
            assert_same_or_nan(got[:, j], want, f"{name} column {j} alpha={alpha} beta={beta}")
    A.free()


def tiny_damped_graph(n=60, seed=41):
    """Two entries of 0.3 per row, run with beta = 0.2 (y is the input vector after the first launch): a finite start
    shrinks by 0.8 per launch until two iterates differ by less than delta.  beta != 0, so y is read like the oracle reads
    it -- with beta == 0 the engine skips y (semiring.hip.h, epilogue) where the oracle's NaN * 0 is a NaN."""
    rng = np.random.default_rng(seed)
    rp = (2 * np.arange(n + 1)).astype(np.int32)
    ci = np.stack([(np.arange(n) + 1) % n, rng.integers(0, n, n)], axis=1).reshape(-1).astype(np.int32)
    return rp, ci, np.full(2 * n, 0.3, np.float32), n


def test_nan_never_converges_in_iterate(eng, plan):
    """differs() is !(|in - out| < delta): a NaN keeps the loop going to max_iters, as in the oracle."""
    rp, ci, va, n = tiny_damped_graph()
    x0 = np.ones(n, np.float32)
    x0[7] = np.nan
    want, w_it, w_conv = O.iterate(PT, rp, ci, va, x0, x0, 1.0, 0.2, 1e-4, 5)
    assert (w_it, w_conv) == (5, False) and np.isnan(want).any()
    A = eng.upload_csr(n, n, rp, ci, va)
    assert A.plan()[0] == plan.split("-")[0]
    xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
    it, conv, _, _ = eng.iterate(PT, A, xv, yv, sc, 1.0, 0.2, delta=1e-4, max_iters=5)
    got = xv.download(np.float32)
    for v in (xv, yv, sc):
        v.free()
    A.free()
    assert (it, conv) == (5, False)
    # 0.3 * a + 0.3 * b is the same in either order: bit for bit
    assert_same_or_nan(got, want, f"sh_iterate with a NaN start, {plan}")


def test_only_the_nan_column_runs_on_in_iterate_multi(eng):
    rp, ci, va, n = tiny_damped_graph()
    width, cap = 4, 60
    starts = [np.ones(n, np.float32), np.full(n, 100.0, np.float32), np.ones(n, np.float32), np.full(n, 1e-3, np.float32)]
    starts[2][7] = np.nan
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    single = []
    for x0 in starts:
        xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
        it, conv, _, _ = eng.iterate(PT, A, xv, yv, sc, 1.0, 0.2, delta=1e-4, max_iters=cap)
        single.append((xv.download(np.float32), it, conv))
        for v in (xv, yv, sc):
            v.free()
        want, w_it, w_conv = O.iterate(PT, rp, ci, va, x0, x0, 1.0, 0.2, 1e-4, cap)
        assert (it, conv) == (w_it, w_conv)
        assert_same_or_nan(single[-1][0], want, "sh_iterate vs the oracle")
    assert [s[2] for s in single] == [True, True, False, True] and single[2][1] == cap
    assert len({s[1] for s in single}) == 4 and max(s[1] for s in single[:2] + single[3:]) < cap
    X0 = interleave(starts, np.float32)
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0)
    launches, iters, conv, _, _ = eng.iterate_multi(PT, A, xv, yv, sc, 1.0, 0.2, width, delta=1e-4, max_iters=cap)
    got = xv.download(np.float32, shape=(n, width))
    for v in (xv, yv, sc):
        v.free()
    A.free()
    assert launches == cap and iters == [s[1] for s in single] and conv == [s[2] for s in single]
    for j in range(width):
        assert_same_or_nan(got[:, j], single[j][0], f"column {j} vs its single run")
