"""tests/truss_ref.py, the reference the GPU tests of sh_truss compare with, is pinned here without a GPU: its model of the
kernels' schedule against the plain serial peel, against the definition of a truss number, against the host gold
(hostlib.truss_numbers, Wang-Cheng) and against the triangle total of tri_ref; the records of the schedule (rounds,
levels, max_truss) on the cases the GPU tests run are asserted; and three deliberately broken rules are shown to give
a wrong answer on the small graphs that isolate the clauses of the rule, so those graphs tell right from wrong."""
import os
import re

import numpy as np
import pytest

import core_ref as K
import tri_ref as T
import truss_ref as R
import wcc_ref as W
from conftest import ROOT
from sparseharness_amd import hostlib as H

PATTERNS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "empty": lambda: (5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "path": lambda: W.path(4096),
    "K300,200": lambda: T.bipartite(300, 200),
    "pattern": T.pattern,
    "noise": lambda: T.with_noise(*T.pattern()),
    "upper": lambda: T.upper_only(*T.pattern()),
    "lower": lambda: T.lower_only(*T.pattern()),
    "pattern5": lambda: T.pattern(300, 6000, 5),
    "K9": lambda: T.complete(9),
    "K60": lambda: T.complete(60),
    "cliques": lambda: K.cliques(2, 12),
    "friendship": lambda: T.friendship(500),
    "tgrid32": lambda: T.triangulated_grid(32),
    "k5_ear": R.k5_ear,
    "k5_ear2": R.k5_ear2,
    "two_hubs9": lambda: R.two_hubs(9),
    "hub_pair-first": lambda: R.hub_pair(40, "first")[:4],
    "hub_pair-middle": lambda: R.hub_pair(41, "middle")[:4],
    "hub_pair-last": lambda: R.hub_pair(40, "last")[:4],
    "rmat10": lambda: (1 << 10,) + H.rmat(10, seed=40),
}
# too large for the serial peel and the definition check in a test: the host gold and the records alone
LARGE = {
    "tgrid": lambda: T.triangulated_grid(128),
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
}
# name -> (M, triangles, max_truss, rounds, levels); None: not asserted
RECORDS = {
    "pattern": (5910, 801, 3, 4, 2),
    "pattern5": (5611, 8706, 5, 35, 4),
    "tgrid": (48_641, 32_258, 3, 128, 1),
    "cliques": (None, None, 12, 11, 11),
    "rmat10": (10_570, None, 30, 132, 29),
    "rmat12": (48_554, 485_410, 50, 284, 43),
}
_got = {}


def case(name):
    if name not in _got:
        m = (PATTERNS.get(name) or LARGE[name])()
        _got[name] = (m, R.peel(*m))
    return _got[name]


def agrees_with_host_gold(m, r):
    eu, ev, sup, truss, edges = H.truss_numbers(*m[1:])
    return (edges == r["M"] and np.array_equal(eu, r["edge_u"]) and np.array_equal(ev, r["edge_v"])
            and np.array_equal(sup, r["support"]) and np.array_equal(truss, r["truss"]))


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reference_four_ways(name):
    m, r = case(name)
    assert r["complete"] and len(r["truss"]) == r["M"] == len(r["support"])
    assert np.array_equal(R.serial(*m), r["truss"]), "the serial peel disagrees"
    assert R.holds_by_definition(*m, r["truss"]), "the definition does not hold"
    assert agrees_with_host_gold(m, r), "the host gold disagrees"
    tri, deg, edges = T.counts(*m)
    assert edges == r["M"] and int(r["support"].sum()) == 3 * (int(tri.sum()) // 3) == 3 * r["triangles"]
    assert int(r["size"].sum()) == r["M"] and len(r["k"]) == r["rounds"] == len(r["size"]) == len(r["walked"])
    assert r["levels"] == len(np.unique(r["truss"])) and r["max_truss"] == (int(r["truss"].max()) if r["M"] else 0)
    assert (np.diff(r["k"]) >= 0).all()
    # the edge ids: the sorted unique pairs u < v
    code = r["edge_u"].astype(np.int64) * max(m[0], 1) + r["edge_v"]
    assert (r["edge_u"] < r["edge_v"]).all() and (np.diff(code) > 0).all()


@pytest.mark.parametrize("name", sorted(LARGE))
def test_large_cases_against_the_host_gold(name):
    m, r = case(name)
    assert r["complete"] and agrees_with_host_gold(m, r)
    tri, deg, edges = T.counts(*m)
    assert edges == r["M"] and int(tri.sum()) // 3 == r["triangles"]


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_records_of_the_schedule(name):
    m, r = case(name)
    edges, triangles, max_truss, rounds, levels = RECORDS[name]
    assert edges is None or r["M"] == edges
    assert triangles is None or r["triangles"] == triangles
    assert (r["max_truss"], r["rounds"], r["levels"]) == (max_truss, rounds, levels)
    if name == "tgrid":
        assert (r["truss"] == 3).all()


def test_definition_check_refuses_wrong_vectors():
    m, r = case("pattern5")
    assert not R.holds_by_definition(*m, np.maximum(r["truss"] - 1, 2))     # too small somewhere
    up = r["truss"].copy()
    up[int(np.argmin(up))] += 1
    assert not R.holds_by_definition(*m, up)                                # too large in one place
    m, r = case("K9")
    assert (r["truss"] == 9).all() and not R.holds_by_definition(*m, r["truss"] + 1)


def test_closed_forms():
    assert (case("K60")[1]["truss"] == 60).all() and case("K60")[1]["rounds"] == 1
    assert (case("path")[1]["truss"] == 2).all() and case("path")[1]["rounds"] == 1
    assert (case("K300,200")[1]["truss"] == 2).all() and case("K300,200")[1]["triangles"] == 0
    assert (case("friendship")[1]["truss"] == 3).all() and case("friendship")[1]["triangles"] == 500
    r = case("k5_ear")[1]
    assert r["truss"].tolist() == [5, 5, 5, 5, 3, 5, 5, 5, 3, 5, 5, 5] and r["size"].tolist() == [2, 10]
    r = case("k5_ear2")[1]
    ends = list(zip(r["edge_u"].tolist(), r["edge_v"].tolist()))
    assert [ends[e] for e in np.flatnonzero(r["truss"] == 3)] == [(0, 5), (1, 5), (1, 6), (5, 6)]
    assert (r["truss"][[ends.index(p) for p in ((0, 1), (2, 4), (3, 4))]] == 5).all()
    assert r["size"].tolist() == [3, 1, 10]        # {1, 5} is settled one round after {0, 5}
    for L in (9, 100):
        r = R.peel(*R.two_hubs(L))
        assert (r["truss"] == 3).all() and r["support"][0] == L and r["size"].tolist() == [2 * L, 1]
        assert r["walked"].tolist() == [4 * L, L + 1]
    for where in ("first", "middle", "last"):
        n, rp, ci, va, (u, v, w) = R.hub_pair(40, where)
        r = R.peel(n, rp, ci, va)
        assert r["size"].tolist() == [80, 1, 20] and r["k"].tolist() == [2, 3, 5]
        ptr, col, deg, _ = K.lists_of(n, rp, ci, va)
        for hub in (u, v):                      # where w stands in the hubs' lists of 45 entries
            at = int(np.searchsorted(col[ptr[hub]:ptr[hub + 1]], w))
            assert deg[hub] == 45
            assert at == 0 if where == "first" else at == 44 if where == "last" else 10 < at < 35


# ---- the small graphs tell the rule of the kernels from broken ones
WRONG_ON = {
    "k5_ear": ("double", "never"),
    "k5_ear2": ("keep-gone",),
    "two_hubs9": ("never",),
}


@pytest.mark.parametrize("name", sorted(WRONG_ON))
def test_broken_rules_give_wrong_truss_numbers(name):
    m, r = case(name)
    for rule in WRONG_ON[name]:
        broken = R.peel(*m, rule=rule)
        assert not np.array_equal(broken["truss"], r["truss"]), rule
        assert not R.holds_by_definition(*m, broken["truss"]), rule
    assert np.array_equal(R.peel(*m, rule="right")["truss"], r["truss"])


def test_cut_short_leaves_unsettled_edges_at_zero():
    m, full = case("tgrid32")
    part = R.peel(*m, max_rounds=5)
    assert part["complete"] is False and part["rounds"] == 5
    done = part["truss"] != 0
    assert done.any() and not done.all() and np.array_equal(part["truss"][done], full["truss"][done])
    assert int(part["size"].sum()) == int(done.sum()) and np.array_equal(part["size"], full["size"][:5])


def test_classes_match_the_kernels():
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "truss.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1)) for k in ("TRUSS_SHORT", "TRUSS_PIECE")}
    assert (const["TRUSS_SHORT"], const["TRUSS_PIECE"]) == (R.SHORT, R.PIECE)
