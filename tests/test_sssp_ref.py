"""What keeps tests/test_sssp_gpu.py honest, checked without a GPU: the numpy reference of sh_sssp (tests/sssp_ref.py)
  1. equals the oracle's own loop (O.iterate on (min,+), delta tiny) bit for bit on the five golden matrices and on
     minplus_ref's real-weight grid and R-MAT-15,
  2. stays inside the float64 path bound of minplus_ref on those two graphs,
  3. is reached, bit for bit, by a push-order bucketed search over a random edge order with a random delta (the claim
     the engine's freedom rests on: the fixed point does not depend on the order of the relaxations),
  4. can fail: a pred that takes the smallest column without the bit test, and a dist added up in float64, are caught.
"""
import numpy as np
import pytest

import minplus_ref as M
import sssp_ref as S
from conftest import MATRICES, mtx
from oracle import oracle as O

MP = O.MIN_PLUS_F32
CASES = MATRICES + list(M.GRAPHS)
_cache = {}


def case(name):
    """(n, row_ptr, col_idx, float32 values) of a matrix."""
    if name not in _cache:
        if name in M.GRAPHS:
            rp, ci, va, n = M.graph(name)
        else:
            rows, cols, _, rp, ci, va = O.mm_load(mtx(name))
            assert rows == cols
            n = rows
        _cache[name] = (n, rp, ci, np.ascontiguousarray(va, np.float32))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_the_oracle_loop(name):
    n, rp, ci, va = case(name)
    for source in (0,) if name in MATRICES else M.sources(name):
        x0 = M.start_vector(n, source)
        dist, pred, reached, _ = S.sssp(rp, ci, va, x0)
        want, it, conv = O.iterate(MP, rp, ci, va, x0, x0, 0.0, 0.0, 1e-300, n + 1)
        assert conv
        np.testing.assert_array_equal(M.bits(dist), M.bits(want))
        assert reached == int((want < M.FLT_MAX).sum())
        assert pred[source] == -1 and ((pred >= 0) == ((dist < M.FLT_MAX) & (np.arange(n) != source))).all()


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_reference_is_inside_the_float64_path_bound(name):
    n, rp, ci, va = case(name)
    for source in M.sources(name):
        x0 = M.start_vector(n, source)
        dist, launches = S.fixed_point(rp, ci, va, x0)
        D, hops = M.float64_sssp(rp, ci, va, source)
        M.assert_within_path_bound(dist, D, hops, launches, what=f"sssp_ref {name} source {source}")


@pytest.mark.parametrize("name", CASES)
def test_a_push_order_search_reaches_the_same_bits(name):
    n, rp, ci, va = case(name)
    rng = np.random.default_rng(123 + len(name))
    x0 = M.start_vector(n, 0)
    x0[rng.integers(1, n, 2)] = [2.5, -0.75]            # further sources with offsets, one of them negative
    dist, _ = S.fixed_point(rp, ci, va, x0)
    _, _, w = S.edges_of(n, rp, ci, va)
    lo, hi = max(float(w.mean()), 1e-3), max(float(w.max()), 2e-3) * 20.0      # (from a weight's size to one bucket for nearly all)
    for delta in (float(np.exp(rng.uniform(np.log(lo), np.log(hi)))), np.inf):
        got = S.push_bellman_ford(rp, ci, va, x0, rng, delta)
        np.testing.assert_array_equal(M.bits(got), M.bits(dist), err_msg=f"{name} delta {delta}")


@pytest.mark.parametrize("name", list(M.GRAPHS))
def test_pred_walks_to_a_root_where_weights_move_the_sum(name):
    n, rp, ci, va = case(name)
    x0 = M.start_vector(n, M.sources(name)[0])
    dist, pred, reached, _ = S.sssp(rp, ci, va, x0)
    c, r, w = S.edges_of(n, rp, ci, va)
    assert (dist[c] + w > dist[c])[dist[c] < M.FLT_MAX].all()     # every weight moves the sum: pred is a forest
    assert S.walk_to_roots(dist, pred) >= 3 and reached > n // 2


def test_the_mutants_are_caught():
    n, rp, ci, va = case("grid")
    x0 = M.start_vector(n, 0)
    dist, pred, _, _ = S.sssp(rp, ci, va, x0)
    loose, _ = S.predecessors(n, rp, ci, va, x0, dist, without_bit_test=True)
    assert (loose != pred).mean() > 0.2                           # the smallest neighbour is not the one the path came through
    with pytest.raises(AssertionError):
        S.walk_to_roots(dist, loose)
    wide = S.float64_mutant(rp, ci, va, x0)
    assert (M.bits(wide) != M.bits(dist)).mean() > 0.2            # one rounding per launch is not one rounding per edge


def test_zero_weights_and_infinite_weights():
    """A stored zero is an edge of weight 0 (and may close a pred cycle-free tie); an infinite weight is no edge."""
    rp = np.array([0, 0, 1, 2, 3, 4], np.int32)                   # 0 -> 1 (0.0), 1 -> 2 (-0.0), 2 -> 3 (inf), 3 -> 4 (1.0)
    ci = np.array([0, 1, 2, 3], np.int32)
    va = np.array([0.0, -0.0, np.inf, 1.0], np.float32)
    c, r, w = S.edges_of(5, rp, ci, va)
    assert len(c) == 3 and M.bits(w).tolist() == [0, 0, 0x3F800000]
    dist, pred, reached, outdeg = S.sssp(rp, ci, va, M.start_vector(5, 0))
    assert M.bits(dist).tolist() == [0, 0, 0, S.FLT_MAX_BITS, S.FLT_MAX_BITS]
    assert pred.tolist() == [-1, 0, 1, -1, -1] and (reached, outdeg) == (3, 2)
