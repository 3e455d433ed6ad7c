"""tests/scc_ref.py is right (no GPU): its Tarjan against a boolean transitive closure and against components known by
construction, its model of sh_scc's schedule against its Tarjan under all four (trim, pivot) settings, the host gold
(hostlib.scc_labels) against both, and the round counts the pattern makers promise."""
import numpy as np
import pytest

import graph_patterns as P
import scc_ref as S
from sparseharness_amd import hostlib as H


def closure_labels(n, src, dst):
    reach = np.eye(n, dtype=bool)
    reach[src, dst] = True
    for k in range(n):   # Warshall
        reach |= np.outer(reach[:, k], reach[k, :])
    both = reach & reach.T
    return np.array([np.nonzero(both[v])[0].max() for v in range(n)], np.int32)


def test_tarjan_against_the_transitive_closure():
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 61))
        m = int(rng.integers(0, 3 * n + 1))
        src, dst = rng.integers(-2, n + 2, m), rng.integers(0, n, m)      # some columns outside the matrix
        va = np.where(rng.random(m) < 0.15, 0.0, 1.0).astype(np.float32)  # some stored zeros
        rp, ci, va = S._csr(n, src, dst, va)
        s, d = S.edges_of(n, rp, ci, va)
        want = closure_labels(n, s, d)
        np.testing.assert_array_equal(S.components(n, rp, ci, va), want)
        np.testing.assert_array_equal(H.scc_labels(rp, ci, va), want)


def test_tarjan_finds_the_planted_blocks():
    for seed in (3, 4, 5):
        n, rp, ci, va, want = S.planted(seed)
        np.testing.assert_array_equal(S.components(n, rp, ci, va), want)
        np.testing.assert_array_equal(H.scc_labels(rp, ci, va), want)
        sizes = np.bincount(want)
        assert sorted(sizes[sizes > 0].tolist()) == sorted(S.PLANTED_BLOCKS) and (sizes >= 2).sum() >= 5


def random_digraph(n, m, seed):
    rng = np.random.default_rng(seed)
    return (n,) + S._csr(n, rng.integers(0, n, m), rng.integers(0, n, m))


def ragged():
    rng, rp, ci = P.ragged_pattern()
    return len(rp) - 1, rp, ci, np.where(rng.random(len(ci)) < 0.1, 0.0, 1.0).astype(np.float32)


def edges():
    rp, ci = P.edges_pattern()
    return len(rp) - 1, rp, ci, np.ones(len(ci), np.float32)


GRAPHS = {
    "planted": lambda: S.planted()[:4],
    "descending": lambda: S.cycle_chain(descending=True),
    "ascending": lambda: S.cycle_chain(descending=False),
    "path": S.path,
    "ragged": ragged,
    "edges": edges,
    "random5200": lambda: random_digraph(4000, 5200, 21),
    "random8000": lambda: random_digraph(4000, 8000, 22),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_schedule_gives_tarjans_labels_under_every_setting(name):
    n, rp, ci, va = GRAPHS[name]()
    want = S.components(n, rp, ci, va)
    np.testing.assert_array_equal(H.scc_labels(rp, ci, va), want)
    print(name, "components", len(np.unique(want)), "largest", np.bincount(want).max())
    for trim in (0, 1):
        for pivot in (0, 1):
            comp, kinds, sizes = S.schedule(n, rp, ci, va, trim, pivot)
            np.testing.assert_array_equal(comp, want, err_msg=f"{name} trim={trim} pivot={pivot}")
            assert sum(sizes) == n and all(s > 0 for s in sizes) and kinds.count(1) <= pivot
            assert trim or 0 not in kinds
            print(name, trim, pivot, "rounds", len(kinds), "colouring", kinds.count(2))


def test_round_counts_of_the_pattern_makers():
    for k, length in ((12, 20), (40, 50)):
        n, rp, ci, va = S.cycle_chain(k, length, descending=True)
        _, kinds, sizes = S.schedule(n, rp, ci, va, 0, 0)
        assert kinds == [2] * k and sizes == [length] * k
        n, rp, ci, va = S.cycle_chain(k, length, descending=False)
        _, kinds, sizes = S.schedule(n, rp, ci, va, 0, 0)
        assert kinds == [2] and sizes == [n]
    n, rp, ci, va = S.path(500)
    assert S.schedule(n, rp, ci, va, 1, 1)[1:] == ([0], [500])
    assert S.schedule(n, rp, ci, va, 0, 0)[1:] == ([2] * 500, [1] * 500)
