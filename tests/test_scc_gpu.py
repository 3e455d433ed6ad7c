"""sh_scc on the GPU: comp against Tarjan (tests/scc_ref.py, pinned by tests/test_scc_ref.py), the kinds and sizes of the
rounds against the numpy model of the schedule, under all four (trim, pivot) settings; the step cap, reuse of a handle, a
graph without rows, the footprint formula, a vector that was filled before, a matrix of self-loops.

Every comparison is exact (==): comp[v] is the largest vertex index of v's component whatever the kernels race on, and
the schedule is fixed.
"""
import numpy as np
import pytest

import graph_patterns as P
import scc_ref as S
from conftest import MATRICES, mtx
from sparseharness_amd import hostlib as H
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

SETTINGS = ((1, 1), (1, 0), (0, 1), (0, 0))
NAMES = MATRICES + ["ragged", "edges", "planted", "descending", "ascending", "path", "rmat15"]
_cache, _want, _sched = {}, {}, {}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def matrix(name):
    """(n, row_ptr, col_idx, values) of a test matrix."""
    if name not in _cache:
        if name == "ragged":       # one row and one column of 20 001 entries: the piece paths
            rng, rp, ci = P.ragged_pattern()
            va = np.where(rng.random(len(ci)) < 0.1, 0.0, 1.0).astype(np.float32)
        elif name == "edges":      # list lengths on the kernels' thresholds
            rp, ci = P.edges_pattern()
            va = np.ones(len(ci), np.float32)
        elif name == "planted":
            _, rp, ci, va, _ = S.planted()
        elif name in ("descending", "ascending"):
            _, rp, ci, va = S.cycle_chain(descending=name == "descending")
        elif name == "path":
            _, rp, ci, va = S.path(500)
        elif name == "rmat15":
            rp, ci, va = H.rmat(15, seed=40)
        elif name == "rmat17":     # long rows and long out-lists
            rp, ci, va = H.rmat(17, seed=40)
        elif name == "loops":
            n = 1000
            rp, ci, va = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)
        else:
            rows, cols, _, rp, ci, va = H.mm_load(mtx(name))
            assert rows == cols
        _cache[name] = (len(rp) - 1, rp, ci, np.ascontiguousarray(va))
    return _cache[name]


def want(name):
    if name not in _want:
        _want[name] = S.components(*matrix(name))
    return _want[name]


def sched(name, trim, pivot):
    if (name, trim, pivot) not in _sched:
        _sched[(name, trim, pivot)] = S.schedule(*matrix(name), trim, pivot)
    return _sched[(name, trim, pivot)]


def run(eng, G, n, trim=1, pivot=1, cap=1 << 20):
    cv = eng.alloc(max(n, 1)).fill(7, np.int32)   # comp pre-filled with 7: it is overwritten in full
    res = eng.scc(G, cv, trim=trim, pivot=pivot, max_steps=cap)
    comp = cv.download(np.int32, n=n)
    cv.free()
    return comp, res


# ------------------------------------------------------------------ 1. every matrix, every setting
@pytest.mark.parametrize("name", NAMES)
def test_components_and_rounds_under_every_setting(eng, name):
    if name == "edges":
        P.assert_edge_lengths(*matrix(name)[1:3])
    components_and_rounds_under_every_setting(eng, name, matrix(name), want(name), lambda trim, pivot: sched(name, trim, pivot))


def components_and_rounds_under_every_setting(eng, name, mat, ref, sched_of):
    n, rp, ci, va = mat
    G = eng.scc_graph(rp, ci, va)
    assert G.edges == len(S.edges_of(n, rp, ci, va)[0])
    for trim, pivot in SETTINGS:
        comp, (components, settled, trimmed, rounds, steps, complete, kinds, sizes, steps_per, edges, ns, total) = \
            run(eng, G, n, trim, pivot)
        _, w_kinds, w_sizes = sched_of(trim, pivot)
        print(f"{name} trim={trim} pivot={pivot}: components {components} trimmed {trimmed} rounds {rounds} steps {steps} "
              f"kinds {kinds[:8].tolist()} sizes {sizes[:8].tolist()} total_ns {total}")
        np.testing.assert_array_equal(comp, ref, err_msg=f"{name} trim={trim} pivot={pivot}")
        assert kinds.tolist() == w_kinds and sizes.tolist() == w_sizes, (name, trim, pivot)
        assert components == int(np.count_nonzero(ref == np.arange(n))) and settled == n and complete
        assert trimmed == sum(s for k, s in zip(w_kinds, w_sizes) if k == 0)
        assert int(sizes.sum()) == n and len(kinds) == len(sizes) == len(steps_per) == len(edges) == len(ns) == rounds
        assert int(steps_per.sum()) <= steps and total >= int(ns.sum())
    G.free()


def test_the_inputs_are_what_they_claim():
    """Structural facts the cases above rely on, from the references alone."""
    ref = want("planted")
    sizes = np.bincount(ref)
    assert (sizes >= 2).sum() >= 5
    np.testing.assert_array_equal(ref, S.planted()[4])
    assert sched("descending", 0, 0)[1] == [2] * 12
    assert sched("ascending", 0, 0)[1] == [2]
    _, kinds, sizes = sched("path", 1, 1)
    assert kinds == [0] and sizes == [500]
    assert sched("path", 0, 0)[1] == [2] * 500


# ------------------------------------------------------------------ 2. long rows and long out-lists, against the host gold
def test_rmat17_against_the_host_gold(eng):
    n, rp, ci, va = matrix("rmat17")
    assert np.diff(rp).max() > 4096 and np.bincount(ci, minlength=n).max() > 4096
    ref = H.scc_labels(rp, ci, va)
    G = eng.scc_graph(rp, ci, va)
    comp, res = run(eng, G, n)
    G.free()
    np.testing.assert_array_equal(comp, ref)
    assert res[0] == int(np.count_nonzero(ref == np.arange(n))) and res[1] == n and res[5]
    print("rmat17: components", res[0], "trimmed", res[2], "rounds", res[3], "steps", res[4], "kinds", res[6].tolist(),
          "sizes", res[7].tolist(), "total_ns", res[11])


# ------------------------------------------------------------------ 3. the step cap
@pytest.mark.parametrize("name,trim,pivot", [("descending", 0, 0), ("planted", 1, 1), ("rmat15", 0, 1)])
def test_a_run_cut_short_reports_only_final_labels(eng, name, trim, pivot):
    """Every one of these runs needs more than three steps whatever the sweeps race on (a round that is no trim round
    is at least four steps: seed, propagation, two claim sweeps); how many it needs in all may differ from run to run,
    so the larger caps assert only what holds either way."""
    n, rp, ci, va = matrix(name)
    ref = want(name)
    G = eng.scc_graph(rp, ci, va)
    _, full = run(eng, G, n, trim, pivot)
    assert full[5] and full[4] >= 4
    for cap in sorted({1, 2, 3, full[4] // 2, full[4] - 1}):
        comp, res = run(eng, G, n, trim, pivot, cap=cap)
        done = comp != -1
        print(f"{name} cap {cap}: settled {res[1]} of {n}, steps {res[4]}, complete {res[5]}")
        if cap <= 3:
            assert not res[5] and not done.all()
        assert res[4] <= cap and (res[5] or res[4] == cap) and res[5] == bool(done.all())
        np.testing.assert_array_equal(comp[done], ref[done])
        assert res[1] == int(done.sum()) and res[0] == int(np.count_nonzero(comp == np.arange(n)))
        assert int(res[7].sum()) == res[1]
    G.free()


# ------------------------------------------------------------------ 4. the handle, the empty graph, the footprint
def test_one_handle_serves_three_calls(eng):
    n, rp, ci, va = matrix("planted")
    G = eng.scc_graph(rp, ci, va)
    first = None
    for trim, pivot in ((1, 1), (0, 0), (1, 1)):
        comp, res = run(eng, G, n, trim, pivot)
        np.testing.assert_array_equal(comp, want("planted"))
        if (trim, pivot) == (1, 1):
            facts = (res[0], res[1], res[2], res[3], res[6].tolist(), res[7].tolist())
            assert first is None or facts == first
            first = facts
    G.free()


def test_a_graph_without_rows(eng):
    G = eng.scc_graph(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert G.edges == 0
    comp, res = run(eng, G, 0)
    assert res[:6] == (0, 0, 0, 0, 0, True) and all(len(a) == 0 for a in res[6:11]) and res[11] == 0
    G.free()


@pytest.mark.parametrize("name", ["matrix", "ragged", "edges"])
def test_footprint_is_the_headers_formula(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.scc_graph(rp, ci, va)
    rows, edges = n, G.edges
    assert G.footprint == 8 * (rows + 1) + 8 * edges + 20 * rows + 32 * (edges // 1024 + 1) + 8 * (edges // 2048 + 1) + 34816
    G.free()


def test_comp_is_overwritten_in_full(eng):
    n, rp, ci, va = matrix("matrix")
    G = eng.scc_graph(rp, ci, va)
    cv = eng.alloc(n + 5).fill(7, np.int32)
    eng.scc(G, cv)
    got = cv.download(np.int32)
    np.testing.assert_array_equal(got[:n], want("matrix"))
    assert (got[n:] == 7).all()   # and nothing beyond the rows
    cv.free()
    G.free()


def test_a_comp_shorter_than_the_rows_is_refused(eng):
    n, rp, ci, va = matrix("matrix")
    G = eng.scc_graph(rp, ci, va)
    cv = eng.alloc(n - 1).fill(7, np.int32)
    with pytest.raises(EngineError, match="comp is shorter") as err:
        eng.scc(G, cv)
    assert err.value.code == abi.SH_ESHAPE
    assert (cv.download(np.int32) == 7).all()   # reported before any device work
    cv.free()
    G.free()


def test_self_loops_alone_are_trimmed(eng):
    n, rp, ci, va = matrix("loops")
    G = eng.scc_graph(rp, ci, va)
    assert G.edges == n
    for trim, pivot in SETTINGS:
        comp, res = run(eng, G, n, trim, pivot)
        np.testing.assert_array_equal(comp, np.arange(n))
        assert res[0] == n and res[1] == n and res[5]
        if trim:
            assert res[2] == n and res[6].tolist() == [0] and res[7].tolist() == [n]
    G.free()
