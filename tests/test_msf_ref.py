"""tests/msf_ref.py is pinned here, without a GPU: Kruskal on KEY against a brute force over all edge subsets on every
labelled graph with up to 5 vertices under tie-heavy weights, the simulator of the round schedule against Kruskal, the
closed forms the GPU tests rely on, and the host gold (host/src/msf_edges.cpp) against the reference."""
import itertools

import numpy as np
import pytest

import msf_ref as F
import wcc_ref as W
from sparseharness_amd import hostlib as H


def _acyclic(n, pairs):
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    for u, v in pairs:
        a, b = find(u), find(v)
        if a == b:
            return False
        parent[a] = b
    return True


def _brute(n, eu, ev, k):
    """The spanning forest whose sorted key vector is smallest, over all edge subsets: a spanning forest is an acyclic
    subset with as many edges as the largest acyclic subset has."""
    M = len(eu)
    key = F.keys_of(k).tolist()
    pairs = list(zip(eu.tolist(), ev.tolist()))
    for size in range(min(M, n - 1), -1, -1):
        best = None
        for sub in itertools.combinations(range(M), size):
            if _acyclic(n, [pairs[e] for e in sub]):
                vec = sorted(key[e] for e in sub)
                if best is None or vec < best[0]:
                    best = (vec, sub)
        if best is not None:
            chosen = np.zeros(M, np.int32)
            chosen[list(best[1])] = 1
            return chosen
    return np.zeros(M, np.int32)


def _graph(n, mask, rng):
    pairs = [(u, v) for u in range(n) for v in range(u + 1, n)]
    have = [pr for i, pr in enumerate(pairs) if mask >> i & 1]
    w = rng.choice(np.array([1, 1, 2], np.float32), size=len(have))   # tie-heavy
    src = np.array([u for u, v in have], np.int64)
    dst = np.array([v for u, v in have], np.int64)
    return W.csr(n, src, dst, w)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_kruskal_on_key_is_the_brute_force_minimum_and_the_simulator_agrees(n):
    rng = np.random.default_rng(100 + n)
    for mask in range(1 << (n * (n - 1) // 2)):
        for _ in range(3 if n < 5 else 1):
            mat = _graph(n, mask, rng)
            eu, ev, weight, k = F.edges(*mat)
            assert len(eu) == bin(mask).count("1")
            want = F.kruskal(n, eu, ev, k)
            assert np.array_equal(want, _brute(n, eu, ev, k)), (n, mask)
            sim = F.schedule(*mat)
            assert sim["complete"] and np.array_equal(sim["in_msf"], want), (n, mask)
            assert np.array_equal(sim["comp"], F.labels(n, eu, ev, np.ones(len(eu), np.int32)))
            assert sim["tree_edges"] == int(want.sum()) == n - sim["components"]
            assert sim["rounds"] <= int(np.log2(n)) + 1


def test_the_order_of_the_bit_patterns():
    f = np.array([-np.inf, -3.5, -1e-45, -0.0, 1e-45, 1e-38, 1.0, np.inf], np.float32)
    bits = np.concatenate([[0xFFC00000, 0xFF800001], f.view(np.uint32), [0x7F800001, 0x7FC00000, 0x7FFFFFFF]]).astype(np.uint32)
    k = F.order_key(bits)   # -NaN < -inf < ... < -0.0 < denormals < ... < +inf < +NaN
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert F.order_key(np.uint32(0)) == 0x80000000 and F.order_key(np.uint32(0x80000000)) == 0x7FFFFFFF


def test_the_smallest_entry_of_an_edge_wins():
    # edge {0, 1} stored as (0, 1) = 5, (1, 0) = 2 and (1, 0) = 3 again; edge {1, 2} once; a loop, a zero, a column outside
    rp = np.array([0, 2, 6, 6], np.int32)
    ci = np.array([1, 0, 0, 0, 2, 7], np.int32)
    va = np.array([5, 9, 2, 3, -1, 1], np.float32)
    eu, ev, weight, k = F.edges(3, rp, ci, va)
    assert eu.tolist() == [0, 1] and ev.tolist() == [1, 2]
    assert weight.view(np.float32).tolist() == [2.0, -1.0]


def test_closed_forms_of_the_schedule():
    sim = F.schedule(*F.ruler_path(1024))
    assert sim["rounds"] == 11 and sim["complete"]
    assert sim["kept"].tolist() == [1023, 511, 255, 127, 63, 31, 15, 7, 3, 1, 0]
    assert sim["hooks"].tolist() == [512, 256, 128, 64, 32, 16, 8, 4, 2, 1, 0]
    assert sim["walked"].tolist() == [1023] + sim["kept"].tolist()[:-1]
    assert sim["in_msf"].all()
    cut = F.schedule(*F.ruler_path(1024), max_rounds=1)
    assert not cut["complete"] and cut["rounds"] == 1 and int(cut["in_msf"].sum()) == 512 and np.all(cut["comp"] == -1)
    assert cut["in_msf"][0::2].all() and not cut["in_msf"][1::2].any()
    sim = F.schedule(*F.weighted(W.grid(64), "unit"))   # ties go by edge id: one round, chains
    assert sim["rounds"] == 2 and sim["hooks"].tolist() == [4095, 0] and sim["depth"][0] > 2
    for ascending in (True, False):
        sim = F.schedule(*F.chain_path(70_001, ascending))   # one round, one chain of depth 70 000
        assert sim["rounds"] == 2 and sim["hooks"].tolist() == [70_000, 0] and sim["depth"][0] >= 65_536
        assert sim["in_msf"].all() and np.all(sim["comp"] == 70_000)


PATTERNS = {
    "ruler": lambda: F.ruler_path(1024),
    "grid-unit": lambda: F.weighted(W.grid(64), "unit"),
    "grid-drawn": lambda: F.weighted(W.grid(32), "drawn", seed=5),
    "islands": F.islands,
    "noise": F.noise,
    "rmat10-drawn": lambda: F.weighted((1 << 10,) + H.rmat(10, seed=40), "drawn", seed=6),
    "rmat10-unit": lambda: F.weighted((1 << 10,) + H.rmat(10, seed=40), "unit"),
    "hub": lambda: F.hub(3000),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_simulator_kruskal_and_host_gold_agree(name):
    mat = PATTERNS[name]()
    n = mat[0]
    eu, ev, weight, k = F.edges(*mat)
    want = F.kruskal(n, eu, ev, k)
    sim = F.schedule(*mat)
    assert sim["complete"] and np.array_equal(sim["in_msf"], want)
    assert np.array_equal(sim["comp"], W.components(*mat))
    geu, gev, gw, gmsf, gcomp, M, components = H.msf_edges(*mat[1:])
    assert M == len(eu) and np.array_equal(geu, eu) and np.array_equal(gev, ev)
    assert np.array_equal(gw, weight) and np.array_equal(gmsf, want)
    assert np.array_equal(gcomp, sim["comp"]) and components == sim["components"]


def test_host_gold_on_special_weights_and_empty_shapes():
    specials = np.array([0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0x00000001, 0x7F800000, 0x7FC00000, 0xBF800000],
                        np.uint32).view(np.float32)
    n, rp, ci, _ = W.grid(8)
    mat = (n, rp, ci, np.resize(specials, len(ci)).astype(np.float32))
    eu, ev, weight, k = F.edges(*mat)
    geu, gev, gw, gmsf, gcomp, M, components = H.msf_edges(*mat[1:])
    assert np.array_equal(gw, weight) and np.array_equal(gmsf, F.kruskal(n, eu, ev, k)) and components == 1
    for n in (0, 1):
        out = H.msf_edges(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        assert out[5] == 0 and out[6] == n and out[4].tolist() == list(range(n))
