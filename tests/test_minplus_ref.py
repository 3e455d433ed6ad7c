"""What keeps tests/test_minplus_gpu.py honest, checked without a GPU:
  1. the two references of one (min,+) launch -- the sequential O.kernel and the order-free numpy restatement of
     tests/minplus_ref.py -- agree bit for bit on every seeded input, so a bit-for-bit demand made of the
     engine rests on the semiring and not on the oracle's loop order,
  2. O.iterate run to an exact fixed point stays inside the float64 path bound on both weighted graphs,
  3. both references can see a lossy layout: weights or x cut to 16 bits change the bits of nearly every reached row
     and push the converged vector out of the bound; dropping fabsf() from the weights changes bits too (the signs of
     the inputs are not decorative),
  4. what Inf, -0.0, subnormals, 2^103 and NaN do to the references (the words a GPU path has to reproduce).
The shares asserted in 3. are floors set below what was measured here against the references (printed by the tests and
recorded in DESIGN.md); they are properties of the inputs, not of the engine.
"""
import numpy as np
import pytest

import float_ref as F
import minplus_ref as M
from oracle import oracle as O

MP = O.MIN_PLUS_F32


def clustered_matrix(n=60_000, seed=11):
    # as tests/test_float_bound.py does: imported late, and that module opens no device by itself (its Engine is a fixture)
    from test_parity_gpu import clustered_matrix as cm
    return cm(n, seed)


GENERATORS = M.generators(clustered_matrix)


@pytest.fixture(scope="module", params=list(GENERATORS))
def data(request):
    c = GENERATORS[request.param]()
    c["name"] = request.param
    return c


def dot_only(c, va, x, **kw):
    """The row minima themselves: y = FLT_MAX, alpha = beta = 0."""
    return M.order_free(c["rp"], c["ci"], va, x, np.full(c["rows"], M.FLT_MAX), 0.0, 0.0, c["cols"], **kw)


# ------------------------------------------------------------------ 1. the references agree
def test_inputs_are_real_signed_and_partly_unreached(data):
    c = data
    for v in (c["va"], c["x"], c["y"]):
        assert (v < 0).any() and (v > 0).any() and np.isfinite(v).all()
    assert (c["va"] != np.round(c["va"])).mean() > 0.9
    for v in (c["x"], c["y"]):
        assert 0.2 < (np.abs(v) == M.FLT_MAX).mean() < 0.4 and (v == -M.FLT_MAX).any() and (v == M.FLT_MAX).any()


@pytest.mark.parametrize("alpha,beta", M.EPILOGUES)
def test_oracle_kernel_equals_the_order_free_reference(data, alpha, beta):
    c = data
    want = O.kernel(MP, c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, vlength=c["cols"])
    ref = M.order_free(c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, c["cols"])
    np.testing.assert_array_equal(M.bits(want), M.bits(ref))
    assert not np.isnan(want).any() and (want >= 0).all()
    if c["name"] == "ragged":
        assert (c["ci"] < 0).any() and (c["ci"] >= c["cols"]).any()


def test_order_free_reference_does_not_depend_on_the_stored_order(data):
    """Every row's entries shuffled: the sequential oracle gives the same words (the premise, on the oracle itself)."""
    c = data
    rng = np.random.default_rng(7)
    row_of = M.rows_of_entries(c["rp"])
    perm = np.lexsort((rng.random(len(row_of)), row_of))
    a = O.kernel(MP, c["rp"], c["ci"], c["va"], c["x"], c["y"], 0.25, 1.5, vlength=c["cols"])
    b = O.kernel(MP, c["rp"], c["ci"][perm], c["va"][perm], c["x"], c["y"], 0.25, 1.5, vlength=c["cols"])
    np.testing.assert_array_equal(M.bits(a), M.bits(b))


# ------------------------------------------------------------------ 2. converged iteration inside the float64 bound
def converged(name, source, va=None):
    rp, ci, w, n = M.graph(name)
    x0 = M.start_vector(n, source)
    # delta = 1e-300: below the smallest float32 difference, so the loop stops at an exact fixed point (delta = 0 never
    # stops: |d| < 0 is false for every d)
    got, it, conv = O.iterate(MP, rp, ci, w if va is None else va, x0, x0, 0.0, 0.0, 1e-300, 5000)
    assert conv
    again = O.kernel(MP, rp, ci, w if va is None else va, got, got, 0.0, 0.0)
    np.testing.assert_array_equal(M.bits(again), M.bits(got))
    return got, it


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_converged_iteration_is_inside_the_float64_path_bound(name):
    rp, ci, va, n = M.graph(name)
    assert (va < 0).mean() > 0.25 and (va != np.round(va)).all()
    for source in M.sources(name):
        got, it = converged(name, source)
        D, hops = M.float64_sssp(rp, ci, va, source)
        assert np.isfinite(D).mean() > 0.5 and it >= 8
        if name == "grid":
            assert it > 150 and np.isfinite(D).all()
        M.assert_within_path_bound(got, D, hops, it, what=f"oracle {name} source {source}")


def test_float64_reference_takes_the_lighter_of_parallel_edges_and_the_magnitude():
    rp = np.array([0, 0, 3, 4], np.int32)                   # 0 -> 1 three times (5, -2, 3), 1 -> 2 (-0.5)
    ci = np.array([0, 0, 0, 1], np.int32)
    va = np.array([5.0, -2.0, 3.0, -0.5], np.float32)
    D, hops = M.float64_sssp(rp, ci, va, 0)
    assert D.tolist() == [0.0, 2.0, 2.5] and hops.tolist() == [0, 1, 2]
    D, hops = M.float64_sssp(rp, ci, va, 2)
    assert np.isinf(D[:2]).all() and hops.tolist() == [-1, -1, 0]
    lo, hi = M.path_bound(D, hops, 3)
    assert lo[0] == hi[0] == float(M.FLT_MAX)
    r = M.path_ratios(np.array([M.FLT_MAX, np.inf, 0.0], np.float32), D, hops, 3)
    assert r.tolist() == [0.0, np.inf, 0.0]


# ------------------------------------------------------------------ 3. sensitivity
# Floors, a margin below the smallest share measured on these inputs (see the printed figures and DESIGN.md):
# one launch, narrowed weights or x: measured 0.973 .. 0.998 of the reached rows change bits;
# fabsf dropped from the weights: measured 0.53 .. 0.60; converged vector, narrowed weights: see FLOOR_OUTSIDE.
FLOOR_BITS, FLOOR_SIGN = 0.95, 0.45


@pytest.mark.parametrize("narrow", list(F.NARROWINGS))
@pytest.mark.parametrize("what", ["values", "x"])
def test_sixteen_bit_floats_change_the_bits_of_one_launch(data, what, narrow):
    c = data
    true = dot_only(c, c["va"], c["x"])
    reached = true < M.FLT_MAX
    cut = F.NARROWINGS[narrow]
    va = cut(c["va"]) if what == "values" else c["va"]
    x = np.where(np.abs(c["x"]) < M.FLT_MAX, cut(c["x"]), c["x"]) if what == "x" else c["x"]   # (unreached stays unreached)
    got = dot_only(c, va, x)
    share = float((M.bits(got) != M.bits(true))[reached].mean())
    print(f"[minplus bound] {c['name']} {what} as {narrow}: {share:.4f} of {int(reached.sum())} reached rows change bits")
    assert reached.sum() > 1000 and share > FLOOR_BITS


def test_dropping_fabsf_from_the_weights_changes_bits(data):
    c = data
    true = dot_only(c, c["va"], c["x"])
    reached = true < M.FLT_MAX
    mutant = dot_only(c, c["va"], c["x"], keep_sign_of_values=True)
    share = float((M.bits(mutant) != M.bits(true))[reached].mean())
    print(f"[minplus bound] {c['name']} without fabsf on the weights: {share:.4f} of {int(reached.sum())} reached rows change bits")
    assert share > FLOOR_SIGN


# Measured: R-MAT 1.000 / 0.997 / 1.000 (bf16 / fp16 / 10-bit mantissa), grid 1.000 / 0.267 / 1.000.  The grid's bound is
# loose by design (k ~ 500 factors) and fp16 rounds to NEAREST, so its errors of either sign average out along a 500-edge
# path and only a quarter of the vertices leave the bound; the truncating formats drift one way and all leave it.
FLOOR_OUTSIDE = {("rmat15", "bf16"): 0.95, ("rmat15", "fp16"): 0.95, ("rmat15", "mant10"): 0.95,
                 ("grid", "bf16"): 0.95, ("grid", "fp16"): 0.15, ("grid", "mant10"): 0.95}


@pytest.mark.parametrize("narrow", list(F.NARROWINGS))
@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_sixteen_bit_weights_leave_the_float64_path_bound(name, narrow):
    """The reference stays the float64 distance on the full-precision weights; only the oracle's weights are narrowed."""
    rp, ci, va, n = M.graph(name)
    source = M.sources(name)[0]
    D, hops = M.float64_sssp(rp, ci, va, source)
    _, it_true = converged(name, source)
    got, it = converged(name, source, F.NARROWINGS[narrow](va))
    r = M.path_ratios(got, D, hops, max(it, it_true))
    far = np.isfinite(D) & (D > 0)
    share = float((r[far] > 1.0).mean())
    print(f"[minplus bound] {name} weights as {narrow}: {share:.4f} of {int(far.sum())} reached vertices outside the bound")
    assert share > FLOOR_OUTSIDE[(name, narrow)]


# ------------------------------------------------------------------ 4. special values, on the references
INF = np.float32(np.inf)


def test_special_values_on_both_references():
    """What a GPU path has to reproduce: an all-Inf row with y = Inf gives the identity seed (FLT_MAX), not Inf; a row
    whose entries all lie outside [0, cols) likewise, weights >= 2^103 or not; -0.0 gives +0; subnormals add exactly."""
    rp = np.array([0, 3, 6, 9, 12, 12], np.int32)
    ci = np.array([0, 1, 2, 0, 1, 2, -1, 7, 5, 3, 4, 3], np.int32)
    tiny = np.float32(2.0 ** -149)
    va = np.array([INF, -INF, INF, 1.5, -2.0 ** 103, 2.0 ** 110, 2.0 ** 103, -2.0 ** 120, 3.0, -0.0, 0.0, 3 * tiny], np.float32)
    x = np.array([1.0, -2.5, -M.FLT_MAX, -0.0, 5 * tiny], np.float32)
    y = np.array([INF, -INF, INF, -M.FLT_MAX, -0.0], np.float32)
    for alpha, beta in M.EPILOGUES + ((-0.0, -0.0),):
        want = O.kernel(MP, rp, ci, va, x, y, alpha, beta, vlength=5)
        np.testing.assert_array_equal(M.bits(want), M.bits(M.order_free(rp, ci, va, x, y, alpha, beta, 5)))
        assert not np.isnan(want).any()
    want = O.kernel(MP, rp, ci, va, x, y, 0.0, 0.0, vlength=5)
    assert M.bits(want)[[0, 2]].tolist() == [0x7F7FFFFF] * 2          # all products Inf / all columns outside: the seed
    assert want[1] == np.float32(2.5)                                # 1.0 + 1.5 beats 2.5 + 2^103 and FLT_MAX + 2^110
    assert M.bits(want)[3] == 0 and M.bits(want)[4] == 0             # |-0.0| + |-0.0| and an empty row with y = -0.0
    sub = O.kernel(MP, rp, ci, va, np.array([1, 1, 1, 7 * tiny, 5 * tiny], np.float32), np.full(5, M.FLT_MAX), 0.0, 0.0, vlength=5)
    assert M.bits(sub)[3] == 5                                       # min(7t + 0, 5t + 0, 7t + 3t) = 5t: exact, not flushed


def test_an_inf_start_on_the_oracle():
    """alpha = 0: min(dot, Inf) <= FLT_MAX replaces the Inf in the first launch.  alpha = Inf: every row keeps |x[r]|, the
    Inf stays, |Inf - Inf| is NaN, `differs` stays true and the loop runs to its cap unconverged."""
    rp, ci, va, n = M.weighted_grid(12, 20, seed=96)
    x0 = M.start_vector(n, 3)
    x0[57] = INF
    want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, np.inf, 0.0, 1e-300, 9)
    assert (it, conv) == (9, False) and np.isinf(want[57]) and (M.bits(want) == M.bits(np.abs(x0))).all()
    first = O.kernel(MP, rp, ci, va, x0, x0, 0.0, 0.0)
    assert np.isfinite(first).all() and first[57] <= M.FLT_MAX
    clean = M.start_vector(n, 3)
    want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, 0.0, 0.0, 1e-300, 500)
    ref, r_it, r_conv = O.iterate(MP, rp, ci, va, clean, clean, 0.0, 0.0, 1e-300, 500)
    assert conv and r_conv and np.array_equal(M.bits(want), M.bits(ref))


def test_rows_reading_nan_is_computed_from_the_inputs():
    rp = np.array([0, 2, 4, 5, 5], np.int32)
    ci = np.array([0, 1, 2, 9, 1], np.int32)
    va = np.array([1, np.nan, 1, 1, 1], np.float32)
    x = np.array([1, 1, np.nan], np.float32)
    y = np.array([0, 0, 0, np.nan], np.float32)
    assert M.rows_reading_nan(rp, ci, va, x, y, 3).tolist() == [True, True, False, True]
    clean = ~M.rows_reading_nan(rp, ci, va, x, y, 3)
    want = O.kernel(MP, rp, ci, va, x, y, 0.0, 0.0, vlength=3)
    assert not np.isnan(want[clean]).any()
    np.testing.assert_array_equal(M.bits(want[clean]), M.bits(M.order_free(rp, ci, va, x, y, 0.0, 0.0, 3)[clean]))


def test_rows_that_read_no_nan_keep_their_bits_on_the_references():
    """The NaN input of the GPU tests: the exempt set (from the inputs alone) is under 1 % of the ragged matrix' rows and
    holds none of its long rows (asserted by M.nan_case); every other row has the same, non-NaN word on both references,
    in stored order and with every row's entries shuffled."""
    c = GENERATORS["ragged"]()
    rp, ci, va, x, y, exempt = M.nan_case(c)
    assert np.isnan(va).sum() == 10 and np.isnan(x).sum() == 1 and np.isnan(y).sum() == 3
    rng = np.random.default_rng(8)
    row_of = M.rows_of_entries(rp)
    perm = np.lexsort((rng.random(len(row_of)), row_of))
    for alpha, beta in M.EPILOGUES:
        want = O.kernel(MP, rp, ci, va, x, y, alpha, beta, vlength=c["cols"])
        assert not np.isnan(want[~exempt]).any()
        ref = M.order_free(rp, ci, va, x, y, alpha, beta, c["cols"])
        np.testing.assert_array_equal(M.bits(want[~exempt]), M.bits(ref[~exempt]))
        other = O.kernel(MP, rp, ci[perm], va[perm], x, y, alpha, beta, vlength=c["cols"])
        np.testing.assert_array_equal(M.bits(want[~exempt]), M.bits(other[~exempt]))
