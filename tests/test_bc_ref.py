"""The references of sh_bc pin one another (no GPU needed): tests/bc_ref.py's ordered (numpy float64 in the header's
summation order) lies within bound's gamma_k of exact (fractions), the host gold hostlib.bc_scores equals ordered bit for
bit, closed forms hold with ==, sigma's three regimes (exact, rounded, inf) show in sigma_max, and a reference that sums
in another order, lets duplicates count or counts the source is noticed."""
from fractions import Fraction

import numpy as np
import pytest

import bc_ref as B
import graph_patterns as P
import small_graphs_ref as S
from sparseharness_amd import hostlib as H


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def host(mat, sources, bc=None):
    bc, sigma, level, depth, reached, smax, edges = H.bc_scores(*mat[1:], sources, bc=bc)
    return dict(bc=bc, sigma=sigma, level=level, depth=depth, reached=reached, sigma_max=smax, edges=edges)


def same(got, want, nan_ok=False):
    """Every output equal: float64 by bit pattern (nan_ok: a NaN stands where a NaN stands, whatever its sign and payload,
    which IEEE leaves open)."""
    for f in ("bc", "sigma", "sigma_max"):
        g, w = np.asarray(got[f], np.float64), np.asarray(want[f], np.float64)
        if nan_ok:
            assert np.array_equal(np.isnan(g), np.isnan(w)), f
            g, w = np.where(np.isnan(g), 0.0, g), np.where(np.isnan(w), 0.0, w)
        assert np.array_equal(bits(g), bits(w)), f
    for f in ("level", "depth", "reached", "edges"):
        assert np.array_equal(got[f], want[f]), f


def within_bound(mat, sources, got):
    want, k = B.exact(mat, sources), B.bound(mat, sources)
    for v in range(mat[0]):
        err = abs(Fraction(float(got[v])) - want[v])
        assert err <= B.gamma(k[v]) * want[v], (v, float(got[v]), want[v], k[v])
        if k[v] == 0:
            assert err == 0


def test_every_digraph_of_four_vertices():
    """ordered within the bound of exact, and the host gold == ordered, from all four sources in two orders."""
    A = S.all_digraphs(4, loops=False)
    assert len(A) == 4096
    for g in range(len(A)):
        mat = B.digraph4(A[g])
        for sources in ((0, 1, 2, 3), (3, 1)):
            o = B.ordered(mat, sources)
            same(host(mat, sources), o)
            if sources == (0, 1, 2, 3) or g % 16 == 0:
                within_bound(mat, sources, o["bc"])


def test_the_union_of_the_small_graphs_is_the_small_graphs():
    """Side by side in one matrix (as the device gets them) the graphs keep their scores: a seeded draw of 64 of them
    against each one alone, and all 4096 with every vertex a source through the host gold."""
    A = S.all_digraphs(4, loops=False)
    pick = np.sort(np.random.default_rng(11).choice(len(A), 64, replace=False))
    assert A[pick][:, 0, :].any() and A[pick][:, :, 0].any() and (A[pick].sum(axis=(1, 2)) >= 10).any()   # no row or column left out
    mat = B.graphs4(pick)
    sources = list(range(mat[0]))
    o = B.ordered(mat, sources)
    same(host(mat, sources), o)
    for i, g in enumerate(pick):
        assert np.array_equal(bits(o["bc"][4 * i:4 * i + 4]), bits(B.ordered(B.digraph4(A[g]), (0, 1, 2, 3))["bc"]))
    mat, sources = B.case("graphs4")
    assert mat[0] == 4 * 4096 == len(sources) and np.array_equal(np.diff(mat[1]).reshape(-1, 4), A.sum(axis=2))
    w = B.want("graphs4")
    for g in pick:
        assert np.array_equal(bits(w["bc"][4 * g:4 * g + 4]), bits(B.ordered(B.digraph4(A[g]), (0, 1, 2, 3))["bc"]))


def test_what_the_device_cases_cover():
    """The cases tests/test_bc_gpu.py runs (bc_ref.CASES) hold what they are there for."""
    wide, c = B.wide(), B.constants()
    assert np.isinf(B.want("diamonds1030")["sigma_max"][0]) and np.isnan(B.want("diamonds1030")["bc"]).any()
    assert B.want("diamonds33")["sigma_max"][0] == 3.0 ** 33 < 2.0 ** 53 < B.want("diamonds34")["sigma_max"][0]
    assert B.want("path300")["depth"][0] == 299 > 8 + 16          # more steps than the first two batches hold
    assert B.want("two-levels")["reached"][0] == wide + 2 and wide > c["BC_MAX_BLOCKS"] * 256
    assert B.want("dead-end")["reached"].tolist() == [1, 3, 1]    # a source without out-edges reaches itself
    assert B.want("star65-all")["bc"][0] == 64.0 * 65
    assert not float(B.want("K7,9")["bc"][0]).is_integer()
    assert B.want("graphs4")["depth"].max() == 3 and B.want("graphs4")["reached"].max() == 4   # 4-cycles and K4 among them
    for k in (c["BC_LANE"] - 1, c["BC_LANE"], c["BC_LANE"] + 1, 63, 64, 65, c["BC_PIECE"] - 1, c["BC_PIECE"],
              c["BC_PIECE"] + 1, 2 * c["BC_PIECE"] + 1):
        assert f"star{k}" in B.CASES


def test_closed_forms():
    n = 100
    mat = B.sym_path(n)
    o = B.ordered(mat, range(n))
    assert o["bc"].tolist() == [2.0 * i * (n - 1 - i) for i in range(n)]
    same(host(mat, list(range(n))), o)
    mat = B.star(65)
    o = B.ordered(mat, range(66))
    assert o["bc"].tolist() == [64.0 * 65] + [0.0] * 65
    same(host(mat, list(range(66))), o)
    n = 37
    mat = B.cycle(n)
    o = B.ordered(mat, range(n))
    assert o["bc"].tolist() == [(n - 1) * (n - 2) / 2] * n and o["depth"].tolist() == [n - 1] * n
    same(host(mat, list(range(n))), o)
    within_bound(B.sym_path(12), range(12), B.ordered(B.sym_path(12), range(12))["bc"])


@pytest.mark.parametrize("k", (5, 33, 34, 40))
def test_sigma_is_exact_below_two_to_the_53_and_rounded_above(k):
    mat = B.diamonds(k, 3)
    o = B.ordered(mat, (0,))
    same(host(mat, (0,)), o)
    top = o["sigma_max"][0]
    assert top == o["sigma"][-1] and o["depth"][0] == 2 * k
    if k <= 33:
        assert 3 ** k < 2 ** 53 and int(top) == 3 ** k
        assert [int(o["sigma"][4 * i]) for i in range(k + 1)] == [3 ** i for i in range(k + 1)]
    else:
        assert top > 2.0 ** 53 and int(top) != 3 ** k and abs(Fraction(float(top)) - 3 ** k) <= B.gamma(2 * k) * 3 ** k
    # a middle of the last diamond carries a third of the paths to its end
    assert abs(o["bc"][-2] - 1 / 3) < 1e-15


def test_sigma_overflows_to_inf_and_says_so():
    mat = B.diamonds(1030, 2)
    o = B.ordered(mat, (0,))
    assert o["sigma_max"][0] == np.inf and o["sigma"][3 * 1023] == 2.0 ** 1023 and o["sigma"][3 * 1024] == np.inf
    assert np.isnan(o["bc"]).any()   # inf / inf
    same(host(mat, (0,)), o, nan_ok=True)


def test_inexact_terms_on_a_complete_bipartite_graph():
    mat = B.bipartite(7, 9)
    sources = list(range(16))
    o = B.ordered(mat, sources)
    same(host(mat, sources), o)
    within_bound(mat, sources, o["bc"])
    assert not float(o["bc"][0]).is_integer()   # sixths and eighths: 1/7 and 1/9 are rounded on the way


@pytest.mark.parametrize("source", P.EDGE_SOURCES)
def test_lists_of_every_length_on_the_thresholds(source):
    """From vertex 0 the hubs pull delta over out-lists of every length of EDGE_LENGTHS less one with terms 1 / sigma that
    are not exact; from vertex 8192 they pull sigma over in-lists of those lengths."""
    rp, ci = P.edges_pattern()
    P.assert_edge_lengths(rp, ci)
    mat = B.with_values(rp, ci)
    o = B.ordered(mat, (source,))
    same(host(mat, (source,)), o)
    assert o["reached"][0] > 8192 and o["sigma_max"][0] > 1.0
    if source == 0:
        assert not all(float(x).is_integer() for x in o["bc"][8192:8204])


def test_rmat10_from_sixteen_drawn_sources():
    rp, ci, va = H.rmat(10, seed=40)
    mat = (1 << 10, rp, ci, va)
    sources = np.random.default_rng(5).integers(0, 1 << 10, 16).tolist()
    o = B.ordered(mat, sources)
    same(host(mat, sources), o)
    # the sources cut into two calls give the bits of one call
    first = host(mat, sources[:7])
    assert np.array_equal(bits(host(mat, sources[7:], bc=first["bc"])["bc"]), bits(o["bc"]))
    assert (o["bc"] > 0).sum() > 100


def test_the_references_notice_a_mutant():
    """Summing in another order, letting duplicates count, or counting the source each changes an output."""
    rp, ci = P.edges_pattern()
    inputs = {"K7,9": (B.bipartite(7, 9), list(range(16))), "edges": (B.with_values(rp, ci), [0]),
              "diamonds twice": (B.restored(B.diamonds(5, 3), twice=True), [0]), "path": (B.sym_path(9), [0, 4])}
    changed = {m: [] for m in ("order", "duplicates", "source")}
    for name, (mat, sources) in inputs.items():
        o = B.ordered(mat, sources)
        same(host(mat, sources), o)
        for m in changed:
            x = B.ordered(mat, sources, mutant=m)
            if not all(np.array_equal(bits(x[f]), bits(o[f])) for f in ("bc", "sigma")):
                changed[m].append(name)
    assert "diamonds twice" in changed["duplicates"] and "path" in changed["source"], changed
    assert changed["order"], changed
    # stored twice or in descending order, the graph is the same graph
    mat = B.diamonds(5, 3)
    for other in (B.restored(mat, twice=True), B.restored(mat, reverse=True)):
        same(B.ordered(other, [0]), B.ordered(mat, [0]))
