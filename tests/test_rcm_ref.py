"""tests/rcm_ref.py pinned on the CPU: the serial definition against the level-synchronous simulator on every graph of up
to 5 labelled vertices and on drawn graphs; certify() accepts those orders and rejects single-swap mutants; broken rules
of the simulator are caught; the host gold (sparseharness_amd/host/src/rcm_order.cpp) gives the reference's answer and
records; bandwidth and profile match a brute-force computation.  No GPU is needed."""
import itertools

import numpy as np
import pytest

import msf_ref as M
import rcm_ref as X
import tri_ref as T
import wcc_ref as W
from sparseharness_amd import hostlib as H

SWEEPS = (0, 1, 8)


def every_small_graph():
    for k in range(1, 6):
        for mask in range(1 << (k * (k - 1) // 2)):
            yield X.small(k, mask)


def drawn_graphs(count=60):
    for seed in range(count):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(1, 15))
        yield X.drawn(n, int(rng.integers(0, 2 * n + 1)), seed)


NAMED = {
    "graphs4": X.all_graphs4,
    "stars": lambda: X.stars((7, 8, 9, 63, 64, 65)),
    "path": lambda: W.path(100, order="index"),
    "K7,7": lambda: T.bipartite(7, 7),
    "grid16-shuffled": lambda: X.shuffled(W.grid(16)),
    "rmat8": lambda: (1 << 8,) + H.rmat(8, seed=40),
    "islands": lambda: M.islands(),
    "messy": lambda: T.with_noise(*T.upper_only(*T.pattern(n=60, m=200, seed=5))),
    "lonely": lambda: X.empty(30),
}


def brute_spread(n, rp, ci, va, p):
    """Bandwidth and profile straight from the definition, one vertex and one entry at a time."""
    nb = [set() for _ in range(n)]
    bits = np.ascontiguousarray(va).view(np.uint32)
    for r in range(n):
        for j in range(rp[r], rp[r + 1]):
            c = int(ci[j])
            if 0 <= c < n and c != r and bits[j] != 0:
                nb[r].add(c)
                nb[c].add(r)
    bw = max([abs(int(p[u]) - int(p[v])) for v in range(n) for u in nb[v]] + [0])
    prof = sum(int(p[v]) - min([int(p[v])] + [int(p[u]) for u in nb[v]]) for v in range(n))
    return bw, prof


def same_answer(mat, sweeps, reverse):
    s, lv = X.serial(*mat, sweeps=sweeps, reverse=reverse), X.levels(*mat, sweeps=sweeps, reverse=reverse)
    for f in ("perm", "pos", "level", "roots"):
        assert np.array_equal(s[f], lv[f]), f
    assert s["components"] == lv["components"] and lv["complete"] is True
    assert lv["steps"] == len(lv["kind"]) <= (sweeps + 2) * mat[0]
    assert X.certify(*mat, s["perm"], s["roots"], reverse) is None
    return s, lv


def test_serial_equals_the_level_form_on_every_graph_of_up_to_5_vertices():
    count = 0
    for mat in every_small_graph():
        for sweeps in SWEEPS:
            same_answer(mat, sweeps, 1)
        count += 1
    assert count == 1 + 2 + 8 + 64 + 1024


def test_serial_equals_the_level_form_on_drawn_graphs():
    for mat in drawn_graphs():
        for sweeps, reverse in itertools.product(SWEEPS, (0, 1)):
            same_answer(mat, sweeps, reverse)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_host_gold_equals_the_reference_on_the_named_shapes(name):
    mat = NAMED[name]()
    for sweeps, reverse in ((0, 1), (1, 0), (8, 1)):
        s, lv = same_answer(mat, sweeps, reverse)
        perm, pos, level, bw0, bw1, p0, p1, comps, searches, kinds, sizes, edges = H.rcm_order(
            *mat[1:], sweeps=sweeps, reverse=reverse, records=True)
        assert np.array_equal(perm, s["perm"]) and np.array_equal(pos, s["pos"]) and np.array_equal(level, s["level"])
        assert (bw0, bw1, p0, p1) == (lv["bandwidth_before"], lv["bandwidth_after"], lv["profile_before"], lv["profile_after"])
        assert (comps, searches) == (lv["components"], lv["sweeps_run"])
        assert np.array_equal(kinds, lv["kind"]) and np.array_equal(sizes, lv["size"]) and np.array_equal(edges, lv["edges"])


def test_host_gold_equals_the_reference_on_small_and_drawn_graphs():
    for mat in itertools.chain((X.small(4, mask) for mask in range(64)), drawn_graphs(30)):
        for sweeps in SWEEPS:
            s = X.serial(*mat, sweeps=sweeps)
            got = H.rcm_order(*mat[1:], sweeps=sweeps)
            assert np.array_equal(got[0], s["perm"]) and np.array_equal(got[2], s["level"]) and got[7] == s["components"]


def test_bandwidth_and_profile_match_a_brute_force_computation():
    for mat in itertools.chain(drawn_graphs(20), [NAMED["messy"](), NAMED["islands"](), NAMED["stars"]()]):
        lv = X.levels(*mat)
        assert (lv["bandwidth_before"], lv["profile_before"]) == brute_spread(*mat, np.arange(mat[0]))
        assert (lv["bandwidth_after"], lv["profile_after"]) == brute_spread(*mat, lv["pos"])
        assert H.rcm_order(*mat[1:])[3:7] == (lv["bandwidth_before"], lv["bandwidth_after"], lv["profile_before"], lv["profile_after"])


def test_the_shuffled_grid_gets_its_bandwidth_back():
    """What the reference alone already gives: 16 x 16 comes down to 16, and never goes up."""
    mat = X.shuffled(W.grid(16), seed=1)
    lv = X.levels(*mat)
    assert lv["bandwidth_before"] > 200 and lv["bandwidth_after"] == 16
    assert lv["profile_after"] < lv["profile_before"]


def test_certify_rejects_single_swap_mutants():
    """Swapping two neighbouring positions of a certified order breaks a rule wherever the two differ in what makes the
    order: their parents, their (deg, index), or their component."""
    mat = X.stars((3, 5), path=6)
    s = X.serial(*mat, sweeps=8, reverse=0)
    assert X.certify(*mat, s["perm"], s["roots"], 0) is None
    rejected = 0
    for k in range(mat[0] - 1):
        mutant = s["perm"].copy()
        mutant[[k, k + 1]] = mutant[[k + 1, k]]
        if X.certify(*mat, mutant, s["roots"], 0) is not None:
            rejected += 1
    assert rejected == mat[0] - 1   # every swap: no two neighbours of this order are interchangeable
    assert X.certify(*mat, s["perm"][::-1].copy(), s["roots"], 0) is not None   # the reversed order under reverse = 0
    assert X.certify(*mat, s["perm"][::-1].copy(), s["roots"], 1) is None
    dup = s["perm"].copy()
    dup[0] = dup[1]
    assert X.certify(*mat, dup, s["roots"], 0) == "perm is no permutation"
    assert X.certify(*mat, s["perm"], s["roots"][1:], 0) is not None   # a root that is not one


def test_broken_rules_of_the_level_form_are_caught():
    """The largest adjacent position as the owner, or children in ascending index, give another order on some graph."""
    differs = {"owner": 0, "emit": 0}
    for mat in itertools.chain(drawn_graphs(40), [NAMED["grid16-shuffled"]()]):
        s = X.serial(*mat)
        if not np.array_equal(X.levels(*mat, owner="largest")["perm"], s["perm"]):
            differs["owner"] += 1
        if not np.array_equal(X.levels(*mat, emit="index")["perm"], s["perm"]):
            differs["emit"] += 1
    assert differs["owner"] > 0 and differs["emit"] > 0


def test_a_run_cut_short_keeps_the_numbered_part():
    mat = X.all_graphs4()
    full = X.levels(*mat, sweeps=8)
    for cap in (1, 5, 37, 200, full["steps"] - 1):
        part = X.levels(*mat, sweeps=8, max_steps=cap)
        assert part["complete"] is False and part["steps"] == cap and part["bandwidth_after"] == -1 and part["profile_after"] == -1
        there = part["perm"] >= 0
        assert there.sum() == part["done"] and np.array_equal(part["perm"][there], full["perm"][there])
        assert np.array_equal(part["kind"], full["kind"][:cap]) and np.array_equal(part["size"], full["size"][:cap])
        assert (part["pos"] >= 0).sum() == part["done"] and (part["level"][part["pos"] < 0] == -1).all()
    assert X.levels(*mat, sweeps=8, max_steps=full["steps"])["complete"] is True
