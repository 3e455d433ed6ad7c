"""tests/core_ref.py, the reference the GPU tests of sh_core compare with, is pinned here without a GPU: against an
independent method (the H-index iteration), against the definition of a core number, against the host gold
(hostlib.core_numbers, Batagelj-Zaversnik) and against closed forms; and the records of the schedule with chase == 0
(degeneracy, rounds, levels) on the cases the GPU tests cap their round counts with are asserted, so those caps rest on
something checked."""
import os
import re

import numpy as np
import pytest

import core_ref as R
import tri_ref as T
import wcc_ref as W
from conftest import ROOT
from sparseharness_amd import hostlib as H

PATTERNS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "empty": lambda: (5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "pattern": T.pattern,
    "noise": lambda: T.with_noise(*T.pattern()),
    "upper": lambda: T.upper_only(*T.pattern()),
    "lower": lambda: T.lower_only(*T.pattern()),
    "K9": lambda: T.complete(9),
    "K300": lambda: T.complete(300),
    "K300,200": lambda: T.bipartite(300, 200),
    "path": lambda: W.path(4096),
    "path-random": lambda: W.path(4096, order="random"),
    "tree": R.tree,
    "cycle": lambda: R.cycle(1000),
    "grid": lambda: W.grid(128),
    "tgrid": lambda: T.triangulated_grid(128),
    "friendship": lambda: T.friendship(500),
    "star": lambda: R.star(3000),
    "cliques": R.cliques,
    "isolated": R.isolated,
    "limits": lambda: R.class_limits()[:4],
    "hub": R.big_hub,
    "hub+K9": lambda: R.big_hub(clique=9),
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
    "rmat15": lambda: (1 << 15,) + H.rmat(15, seed=40),
}
_got = {}


def case(name):
    if name not in _got:
        m = PATTERNS[name]()
        _got[name] = (m, R.peel(*m))
    return _got[name]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reference_three_ways(name):
    m, r = case(name)
    n = m[0]
    assert r["complete"] and len(r["core"]) == n
    assert np.array_equal(R.hindex(*m), r["core"]), "the H-index iteration disagrees"
    assert R.holds_by_definition(*m, r["core"]), "the definition does not hold"
    core, deg, edges = H.core_numbers(*m[1:])
    assert np.array_equal(core, r["core"]) and np.array_equal(deg, r["deg"]) and edges == r["M"]
    # the records hang together
    assert r["degeneracy"] == (int(r["core"].max()) if n else 0)
    assert r["levels"] == len(np.unique(r["core"])) and r["rounds"] == len(r["k"])
    assert int(r["size"].sum()) == n and (np.diff(r["k"]) >= 0).all() and (r["size"] > 0).all()
    if n:   # a round settles its list at its k
        per_level = np.bincount(r["k"], weights=r["size"], minlength=r["degeneracy"] + 1).astype(np.int64)
        assert np.array_equal(per_level, np.bincount(r["core"], minlength=r["degeneracy"] + 1))


def test_the_definition_check_refuses_wrong_vectors():
    m, r = case("pattern")
    core = r["core"].copy()
    assert R.holds_by_definition(*m, core)
    top = int(np.argmax(core))
    low = core.copy()
    low[top] -= 1
    high = core.copy()
    high[top] += 1
    assert not R.holds_by_definition(*m, low) and not R.holds_by_definition(*m, high)
    assert not R.holds_by_definition(*m, r["deg"])


def test_closed_forms():
    core = lambda name: case(name)[1]["core"]   # noqa: E731
    assert (core("K9") == 8).all() and (core("K300") == 299).all()
    assert (core("path") == 1).all() and (core("path-random") == 1).all() and (core("tree") == 1).all()
    assert (core("cycle") == 2).all() and (core("grid") == 2).all()
    assert (core("K300,200") == 200).all()
    assert (core("friendship") == 2).all() and (core("star") == 1).all()
    assert case("cliques")[1]["levels"] == 39 and case("cliques")[1]["degeneracy"] == 39
    for a, b in ((3, 7), (7, 3), (1, 5)):
        assert (R.peel(*T.bipartite(a, b))["core"] == min(a, b)).all()
    iso = core("isolated")
    assert (iso[:100] == 2).all() and (iso[100:] == 0).all()
    assert case("empty")[1]["degeneracy"] == 0 and case("empty")[1]["rounds"] == 1 and (core("empty") == 0).all()
    assert case("no-rows")[1]["rounds"] == 0 and case("no-rows")[1]["levels"] == 0
    assert (core("hub") == 1).all()
    c9 = core("hub+K9")
    assert c9[0] == 8 and (c9[1:70_002] == 1).all() and (c9[70_002:] == 8).all()


def test_noise_and_storage_forms_change_nothing():
    want = case("pattern")[1]
    n, rp, ci, va = case("noise")[0]
    assert T.counts(*T.noise_as_edges(n, rp, ci, va))[2] > want["M"]   # (it would change the graph if it counted)
    for form in ("noise", "upper", "lower"):
        got = case(form)[1]
        assert np.array_equal(got["core"], want["core"]) and np.array_equal(got["deg"], want["deg"]) and got["M"] == want["M"]
        for f in ("k", "size", "edges"):
            assert np.array_equal(got[f], want[f])


def test_class_limits_hubs_decide_their_neighbours():
    n, rp, ci, va, hubs = R.class_limits()
    r = R.peel(n, rp, ci, va)
    assert tuple(r["deg"][hubs].tolist()) == R.HUB_DEGREES == (8, 9, 2048, 2049, 4097)
    assert (r["core"][hubs] == 2).all() and r["k"].tolist() == [1, 2, 2, 3]
    assert r["size"][1] == len(hubs)          # level 2 opens with the hubs alone: their neighbours x, y are unsettled
    for h, d in zip(hubs.tolist(), R.HUB_DEGREES):
        x, y = h + 1, h + 6 + d - 2
        assert r["deg"][x] == 3 and r["deg"][y] == 3 and r["core"][x] == 2 and r["core"][y] == 2
        assert (r["core"][h + 2:h + 6] == 3).all()
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "core.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1)) for k in ("CORE_SHORT", "CORE_PIECE")}
    assert (const["CORE_SHORT"], const["CORE_PIECE"]) == (R.SHORT, R.PIECE)


# degeneracy, rounds, levels of the schedule with chase == 0 (None: not asserted)
MEASURED = {
    "rmat12": (65, 125, 51),
    "rmat15": (162, 226, 79),
    "grid": (2, 127, 1),
    "tgrid": (3, 129, 2),
    "path": (1, 2048, 1),
    "pattern": (11, 34, 5),
    "K300": (None, 1, None),
    "K300,200": (None, 2, None),
}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_records_of_the_schedule_without_chase(name):
    r = case(name)[1]
    degeneracy, rounds, levels = MEASURED[name]
    assert r["rounds"] == rounds
    assert degeneracy is None or r["degeneracy"] == degeneracy
    assert levels is None or r["levels"] == levels


def test_cut_short_settles_a_prefix():
    m, full = case("grid")
    part = R.peel(*m, max_rounds=10)
    assert not part["complete"] and part["rounds"] == 10
    done = part["core"] >= 0
    assert int(done.sum()) == int(full["size"][:10].sum()) and (part["core"][~done] == -1).all()
    assert np.array_equal(part["core"][done], full["core"][done])
