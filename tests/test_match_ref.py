"""tests/match_ref.py is pinned here, without a GPU: the simulator of the rounds against the serial definition on every
undirected graph on 5 vertices under tie-heavy and monotone weights and every order, on R-MAT-10 and the patterns of the
GPU tests; the host gold (host/src/greedy_matching.cpp) against the definition; certify() on all of them and on
hand-broken mates; the round bound and the one input that attains it."""
import numpy as np
import pytest

import match_ref as M
import msf_ref as F
import small_graphs_ref as S
import wcc_ref as W
from sparseharness_amd import hostlib as H

ORDERS = [(heavy, seed) for heavy in (0, 1) for seed in (0, 7)]


def _five(weights):
    """Every undirected graph on 5 vertices as (n, eu, ev, k, mat): local edge lists, weights by local edge id, and the
    CSR arrays that store every edge once."""
    A = S.all_undirected(5)
    pairs = [(u, v) for u in range(5) for v in range(u + 1, 5)]
    for g in range(A.shape[0]):
        have = [(u, v) for (u, v) in pairs if A[g, u, v]]
        m = len(have)
        w = {"equal": np.ones(m), "ascending": np.arange(1, m + 1), "descending": np.arange(m, 0, -1)}[weights]
        eu = np.array([u for u, v in have], np.int32)
        ev = np.array([v for u, v in have], np.int32)
        yield 5, eu, ev, F.order_key(w.astype(np.float32).view(np.uint32)), W.csr(5, eu, ev, w.astype(np.float32))


@pytest.mark.parametrize("weights", ["equal", "ascending", "descending"])
def test_rounds_and_greedy_agree_on_every_graph_on_five_vertices(weights):
    most = 0
    for n, eu, ev, k, mat in _five(weights):
        for heavy, seed in ORDERS:
            keys = M.mkeys(k, heavy, seed)
            assert len(np.unique(keys)) == len(keys)
            mate, chosen = M.greedy(n, eu, ev, keys)
            gold = H.greedy_matching(*mat[1:], heavy=heavy, seed=seed)
            assert np.array_equal(gold[0], eu) and np.array_equal(gold[1], ev)
            assert np.array_equal(gold[3], chosen) and np.array_equal(gold[4], mate)
            sim = M.rounds(n, eu, ev, keys)
            assert sim["complete"] and np.array_equal(sim["mate"], mate) and np.array_equal(sim["in_match"], chosen)
            assert M.certify(mate, eu, ev, keys) == ""
            assert sim["rounds"] <= n // 2 + 1 and sim["pairs"] == int((mate > np.arange(n)).sum())
            assert sim["walked"][0] == len(eu) and np.array_equal(sim["walked"][1:], sim["kept"][:-1])
            assert sim["kept"][-1] == 0 and np.all(sim["matched"][:-1] >= 1)
            most = max(most, sim["rounds"])
    assert most == 3   # the bound floor(5 / 2) + 1 is met by some graph on 5 vertices


PATTERNS = {
    "rmat10-drawn": lambda: F.weighted((1 << 10,) + H.rmat(10, seed=40), "drawn", seed=6),
    "rmat10-unit": lambda: F.weighted((1 << 10,) + H.rmat(10, seed=40), "unit"),
    "grid-unit": lambda: F.weighted(W.grid(24), "unit"),
    "islands": F.islands,
    "noise": F.noise,
    "hub": lambda: M.hub(3000),
    "stars-257": lambda: M.stars_and_path(257),
    "path-60": lambda: M.ascending_path(60),
    "packed4-equal": lambda: M.packed4("equal"),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_simulator_definition_and_host_gold_agree(name):
    mat = PATTERNS[name]()
    for heavy, seed in ORDERS + [(1, 1)]:
        n, eu, ev, weight, keys = M.case(mat, heavy, seed)
        mate, chosen = M.greedy(n, eu, ev, keys)
        sim = M.rounds(n, eu, ev, keys)
        assert sim["complete"] and np.array_equal(sim["mate"], mate) and np.array_equal(sim["in_match"], chosen)
        assert M.certify(mate, eu, ev, keys) == ""
        geu, gev, gw, gin, gmate, gM, pairs = H.greedy_matching(*mat[1:], heavy=heavy, seed=seed)
        assert gM == len(eu) and np.array_equal(geu, eu) and np.array_equal(gev, ev) and np.array_equal(gw, weight)
        assert np.array_equal(gin, chosen) and np.array_equal(gmate, mate) and pairs == int(chosen.sum())
        assert sim["rounds"] <= n // 2 + 1


def test_certify_rejects_broken_mates():
    n, eu, ev, weight, keys = M.case(M.ascending_path(8), 0, 0)   # the pairs (0, 1), (2, 3), (4, 5), (6, 7)
    mate, _ = M.greedy(n, eu, ev, keys)
    assert mate.tolist() == [1, 0, 3, 2, 5, 4, 7, 6] and M.certify(mate, eu, ev, keys) == ""
    free = mate.copy()
    free[[2, 3]] = -1
    assert "two free ends" in M.certify(free, eu, ev, keys)
    one_way = mate.copy()
    one_way[3] = -1
    assert "involution" in M.certify(one_way, eu, ev, keys)
    no_edge = np.array([2, 3, 0, 1, 5, 4, 7, 6])
    assert "no edge" in M.certify(no_edge, eu, ev, keys)
    shifted = np.array([-1, 2, 1, 4, 3, 6, 5, -1])   # maximal and valid, but not greedy's: (0, 1) is below (1, 2)
    assert "below both" in M.certify(shifted, eu, ev, keys)
    assert "outside" in M.certify(np.array([1, 0, 3, 2, 5, 4, 8, 6]), eu, ev, keys)
    # heaviest first on the same path: (6, 7), (4, 5), ... is the same set here, but on 7 vertices it is the other one
    n, eu, ev, weight, keys = M.case(M.ascending_path(7), 1, 0)
    mate, _ = M.greedy(n, eu, ev, keys)
    assert mate.tolist() == [-1, 2, 1, 4, 3, 6, 5] and M.certify(mate, eu, ev, keys) == ""
    assert M.certify(np.array([1, 0, 3, 2, 5, 4, -1]), eu, ev, keys) != ""


def test_the_round_bound_is_attained_by_the_ascending_path_and_by_nothing_else_tried():
    for n in (2, 3, 8, 59, 60):
        sim = M.rounds(*_split(M.ascending_path(n), 0, 0))
        assert sim["rounds"] == n // 2 + 1 and sim["matched"].tolist() == [1] * (n // 2) + [0]
    sim = M.rounds(*_split(M.ascending_path(60), 0, 0))
    assert sim["kept"].tolist() == list(range(59, 0, -2)) + [0]
    assert sim["walked"].tolist() == [59] + sim["kept"].tolist()[:-1]
    for heavy, seed in ORDERS:   # the weights differ, so the seed decides nothing; heaviest first pairs the far end first
        assert M.rounds(*_split(M.ascending_path(60), heavy, seed))["rounds"] == 31
    for name in sorted(PATTERNS):
        if name == "path-60":
            continue
        mat = PATTERNS[name]()
        for heavy, seed in ORDERS:
            sim = M.rounds(*_split(mat, heavy, seed))
            assert sim["rounds"] < mat[0] // 2 + 1, name


def _split(mat, heavy, seed):
    n, eu, ev, _, keys = M.case(mat, heavy, seed)
    return n, eu, ev, keys


def test_mkeys_and_the_all_ones_key():
    k = F.order_key(np.array([1.0, 2.0, 2.0, -1.0], np.float32).view(np.uint32))
    assert np.argsort(M.mkeys(k, 0, 0)).tolist() == [3, 0, 1, 2]
    assert np.argsort(M.mkeys(k, 1, 0)).tolist() == [1, 2, 0, 3]
    for seed in (1, 7, 0xDEADBEEF):
        lo = M.mkeys(np.zeros(1 << 12, np.uint32), 0, seed) & np.uint64(0xFFFFFFFF)
        assert len(np.unique(lo)) == 1 << 12
    for y in (0, 1, 0xFFFFFFFF, 0x12345678):
        assert int(M.mix32(np.array([M.unmix32(y)]))[0]) == y
    # seed such that edge 1 of a path of 4 gets lo == 0xFFFFFFFF, its weight the last of the order: its key is all ones,
    # and it is still matched when it is the one kept edge at both its ends
    seed = M.unmix32(0xFFFFFFFF) ^ 1
    last = np.array([0x7FFFFFFF], np.uint32).view(np.float32)[0]
    mat = F.by_edge(W.path(4), np.array([1.0, last, 1.0], np.float32))
    n, eu, ev, weight, keys = M.case(mat, 0, seed)
    assert keys[1] == M.MAX
    assert M.greedy(n, eu, ev, keys)[0].tolist() == [1, 0, 3, 2]
    mat = (4,) + W.csr(4, np.array([1]), np.array([2]), np.array([last], np.float32))[1:]   # edge 0 only: another seed
    n, eu, ev, weight, keys = M.case(mat, 0, M.unmix32(0xFFFFFFFF))
    assert keys.tolist() == [int(M.MAX)]
    sim = M.rounds(n, eu, ev, keys)
    assert sim["mate"].tolist() == [-1, 2, 1, -1] and sim["rounds"] == 2 and M.certify(sim["mate"], eu, ev, keys) == ""


def test_host_gold_on_special_weights_empty_shapes_and_bad_scalars():
    specials = np.array([0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0x00000001, 0x7F800000, 0x7FC00000, 0xBF800000],
                        np.uint32).view(np.float32)
    n, rp, ci, _ = W.grid(8)
    mat = (n, rp, ci, np.resize(specials, len(ci)).astype(np.float32))
    for heavy, seed in ORDERS:
        n, eu, ev, weight, keys = M.case(mat, heavy, seed)
        out = H.greedy_matching(*mat[1:], heavy=heavy, seed=seed)
        assert np.array_equal(out[2], weight) and np.array_equal(out[4], M.greedy(n, eu, ev, keys)[0])
    for n in (0, 1):
        out = H.greedy_matching(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        assert out[5] == 0 and out[6] == 0 and out[4].tolist() == [-1] * n
    with pytest.raises(RuntimeError):
        H.greedy_matching(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), heavy=2)
