"""tests/trsv_ref.py against the host gold and against exact arithmetic (no GPU needed): the numpy restatement of sh_trsv's
definition equals hostlib.trsv_solve bit for bit on every case; on the small cases the computed x satisfies the
componentwise bound of substitution, computed exactly in fractions; the three tiers of the sum are one function."""
from fractions import Fraction

import numpy as np
import pytest

import trsv_ref as T
from sparseharness_amd import hostlib

U = Fraction(1, 2 ** 53)
U32 = Fraction(1, 2 ** 24)


def gamma(k):
    return k * U / (1 - k * U)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_x(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what   # a NaN stands where a NaN stands
    ok = ~np.isnan(want)
    bad = np.nonzero(bits(got)[ok] != bits(want)[ok])[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[ok][bad[:5]].tolist(), want[ok][bad[:5]].tolist())


FIGURES = ("entries", "levels", "max_list", "max_width", "zero_diag", "first_zero")


@pytest.mark.parametrize("f32", (0, 1))
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_the_restatement_equals_the_host_gold_bit_for_bit(name, f32):
    c, w = T.case(name), T.want(name, f32)
    x, level, fig = hostlib.trsv_solve(*c["mat"][1:], c["b"], c["uplo"], c["unit"], f32)
    same_x(x, w["x"], name)
    assert np.array_equal(level, w["level"]), name
    assert fig == {k: w[k] for k in FIGURES}, name


def test_the_cases_are_what_they_are_named_for():
    w = T.want("tiers")
    ln = np.diff(T.lists(T.case("tiers")["mat"], 0, 0)[0])
    assert sorted(ln[ln > 0].tolist()) == sorted([1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4097, 11])
    assert (w["levels"], w["max_width"]) == (3, 4100)
    w = T.want("wide")
    assert w["levels"] == 2 and w["max_width"] > T.MAX_BLOCKS * 256
    assert T.want("path30")["levels"] == 30 > 8 + 16   # more rounds than the analysis' first two batches hold
    assert T.want("path-runs")["levels"] == 2 * T.RUN + 3 and T.want("path-runs-upper")["levels"] == 2 * T.RUN + 3
    for t, name in ((64, "widths64"), (T.THIN, "widths256")):
        assert np.diff(T.want(name)["lstart"]).tolist() == [t - 1, t, t + 1, 1, t + 1]
    w = T.want("dirt")
    assert (w["zero_diag"], w["first_zero"]) == (2, 5) and np.isinf(w["x"][5]) and np.isnan(w["x"][[10, 11]]).all()
    assert np.isfinite(w["x"][[0, 1, 2, 3, 4]]).all() and np.abs(w["x"][:5]).max() < 1e6   # no guard value was read
    assert w["x"][8] == 0.0 and np.signbit(w["x"][8]) and np.isinf(w["x"][9])
    assert T.want("dirt-unit")["zero_diag"] == 0 and T.want("dirt-unit")["first_zero"] == -1
    assert T.want("rows0")["levels"] == 0 and T.want("rows1")["x"].tolist() == [T.case("rows1")["b"][0] / 2.5]
    assert T.want("tri4-lower")["entries"] == 64 * 3 and T.want("tri4-upper")["entries"] == 64 * 3


@pytest.mark.parametrize("name", T.SMALL)
def test_the_componentwise_bound_of_substitution_holds_exactly(name):
    """|b - T x|_r <= gamma_k (|T| |x|)_r with k = len_r + 2 (a term passes through at most len_r - 1 additions that can
    round -- adding +0.0 is exact --, one multiplication, the subtraction and the division; Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., section 8.1: it holds for any order of the sum).  The bound is derived, not
    measured.  With f32 the x handed out is rounded once more: |x32 - x64| <= 2^-24 |x64| adds 2^-24 (|T| |x64|)_r."""
    c = T.case(name)
    w = T.want(name)
    assert np.isfinite(w["x"]).all()
    worst = Fraction(0)
    for r, (res, scale, ln) in enumerate(T.residual_and_scale(c["mat"], c["b"], w["x"], c["uplo"], c["unit"])):
        assert res <= gamma(ln + 2) * scale, (name, r, float(res), float(scale), ln)
        if scale:
            worst = max(worst, res / (gamma(ln + 2) * scale))
    print(name, "largest residual / bound:", float(worst))
    w32 = T.want(name, 1)
    b32 = np.asarray(c["b"], np.float32).astype(np.float64)
    for r, (res, scale, ln) in enumerate(T.residual_and_scale(c["mat"], b32, w32["x"].astype(np.float64), c["uplo"], c["unit"],
                                                              x_in=w32["x64"])):
        assert res <= (gamma(ln + 2) + U32) * scale, (name, "f32", r, float(res), float(scale), ln)


def test_the_exact_solve_agrees_where_the_arithmetic_is_exact():
    """Small integers and powers of two: every product, sum and quotient is exact, so x is the exact solution."""
    mat = T.csr(5, [(0, 0, 1.0), (1, 0, 2.0), (1, 1, 4.0), (2, 1, -3.0), (2, 0, 1.0), (2, 2, 2.0), (3, 3, 0.5), (4, 3, 8.0),
                    (4, 2, -1.0), (4, 2, 2.0), (4, 4, 1.0)])
    b = np.array([3.0, 10.0, -5.0, 1.5, 7.0])
    x = T.exact_solve(mat, b)
    assert [Fraction(float(v)) for v in T.solve(mat, b)["x"]] == x
    assert [Fraction(float(v)) for v in hostlib.trsv_solve(*mat[1:], b)[0]] == x
    up = T.transposed(mat)
    assert [Fraction(float(v)) for v in T.solve(up, b, uplo=1)["x"]] == T.exact_solve(up, b, uplo=1)


LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4097)


@pytest.mark.parametrize("kind", ("drawn", "negative zeros", "cancelling pairs", "mixed zeros"))
def test_the_three_tiers_of_the_sum_are_one_function(kind):
    rng = np.random.default_rng(5)
    for n in LENGTHS:
        if kind == "drawn":
            t = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)
        elif kind == "negative zeros":
            t = np.full(n, -0.0)
        elif kind == "cancelling pairs":
            t = rng.normal(size=n)
            t[1::2] = -t[:2 * (n // 2):2]
        else:
            t = rng.choice([0.0, -0.0, 1.5, -1.5], n)
        pieces = T.sum_pieces(t)
        assert bits(np.float64(T.list_sum(t))) == bits(np.float64(pieces)), (kind, n)
        if n <= T.LANE:
            assert bits(np.float64(T.sum_lane(t))) == bits(np.float64(pieces)), (kind, n)
            assert bits(np.float64(hostlib.trsv_list_sum(t, 1))) == bits(np.float64(pieces)), (kind, n)
        if n <= T.PIECE:   # one piece: a wave's single pass is the same as the walk over pieces with any larger piece
            assert bits(np.float64(T.sum_pieces(t, piece=2 * T.PIECE))) == bits(np.float64(pieces)), (kind, n)
        for tier in (0, 2):
            assert bits(np.float64(hostlib.trsv_list_sum(t, tier))) == bits(np.float64(pieces)), (kind, n, tier)
        if kind == "negative zeros":
            assert pieces == 0.0 and not np.signbit(pieces)   # +0.0 in every tier: a partial starts from +0.0
        # padding with +0.0 entries behind the list changes nothing (what the idle lanes of a wave add)
        assert bits(np.float64(T.sum_pieces(np.concatenate([t, np.zeros((-n) % 64)])))) == bits(np.float64(pieces))


def test_the_plan_is_a_function_of_lstart_thin_and_the_cap():
    ls = [0, 63, 127, 192, 193, 258]
    assert T.plan(ls, 0) == (5, 0, 0)
    assert T.plan(ls, 1) == (5, 1, 1)
    assert T.plan(ls, 63) == (5, 2, 2)            # [63] run, 64 wide, 65 wide, [1] run, 65 wide
    assert T.plan(ls, 64) == (4, 2, 3)            # [63, 64] run, 65 wide, [1] run, 65 wide
    assert T.plan(ls, 65) == (1, 1, 5) and T.plan(ls, None) == (1, 1, 5) and T.plan(ls, -1) == (1, 1, 5)
    path = np.arange(2 * T.RUN + 4)
    assert T.plan(path) == (3, 3, 2 * T.RUN + 3) and T.plan(path, 0) == (2 * T.RUN + 3, 0, 0)
    assert T.plan(path, 1, run=100) == (21, 21, 2051)
    assert T.plan([0]) == (0, 0, 0)
