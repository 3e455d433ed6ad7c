"""sh_wcc on the GPU: comp against the union-find of tests/wcc_ref.py (pinned by tests/test_wcc_ref.py), under
sample = 0, 1, 2 and 5 unless a case says otherwise; against sh_scc on symmetric patterns; the bound on the rounds of a
path, the round cap, reuse of a handle, the per-round arrays, the footprint formula.

Every comparison of labels is exact (==): comp[v] is the largest vertex index of v's weak component whatever the kernels
race on and whatever the sample picks.  The shapes are the smallest at which the kernels can still go wrong: lists on both
sides of the classes' limits (one lane up to 8 entries, the wave up to 2048, pieces beyond), more vertices than one launch
has lanes only where the case needs them (the hubs, the path).
"""
import numpy as np
import pytest

import scc_ref as S
import wcc_ref as W
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

SAMPLES = (0, 1, 2, 5)
_cache, _want = {}, {}


def _loops():
    n = 1000
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)


MAKERS = {
    "empty": lambda: (5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "loops": _loops,
    "noise": lambda: W.with_noise(*W.no_giant()),
    "up": lambda: W.one_way(up=True),
    "down": lambda: W.one_way(up=False),
    "hub-out-largest": lambda: W.hub(where="largest", out=True),
    "hub-out-smallest": lambda: W.hub(where="smallest", out=True),
    "hub-in-largest": lambda: W.hub(where="largest", out=False),
    "hub-in-smallest": lambda: W.hub(where="smallest", out=False),
    "limits-in": lambda: W.class_limits(out=False),
    "limits-out": lambda: W.class_limits(out=True),
    "path-index": lambda: W.path(order="index"),
    "path-reversed": lambda: W.path(order="reversed"),
    "path-random": lambda: W.path(order="random"),
    "grid": lambda: W.grid(128),
    "rmat12": lambda: W.symmetrised(1 << 12, *H.rmat(12, seed=40)),
    "rmat15": lambda: W.symmetrised(1 << 15, *H.rmat(15, seed=40)),
    "rmat15-directed": lambda: (1 << 15,) + H.rmat(15, seed=40),
    "pendants-out": lambda: W.pendants(in_giant_rows=True),
    "pendants-in": lambda: W.pendants(in_giant_rows=False),
    "no-giant": W.no_giant,
    "planted": lambda: S.planted()[:4],
}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def matrix(name):
    if name not in _cache:
        n, rp, ci, va = MAKERS[name]()
        _cache[name] = (n, rp, ci, np.ascontiguousarray(va))
    return _cache[name]


def want(name):
    """The reference's labels: computed once per matrix, shared, never written to."""
    if name not in _want:
        _want[name] = W.components(*matrix(name))
        _want[name].setflags(write=False)
    return _want[name]


def run(eng, G, n, sample=2, cap=1 << 20):
    cv = eng.alloc(max(n, 1)).fill(7, np.int32)   # comp pre-filled with 7: it is overwritten in full
    res = eng.wcc(G, cv, sample=sample, max_rounds=cap)
    comp = cv.download(np.int32, n=n)
    cv.free()
    return comp, res


def check(eng, name, samples=SAMPLES, mat=None, ref=None):
    """comp == the reference under every sample, and what the counts must satisfy; -> the results by sample."""
    n, rp, ci, va = matrix(name) if mat is None else mat
    ref = want(name) if ref is None else ref
    largest = int(np.bincount(ref).max())
    G = eng.wcc_graph(rp, ci, va)
    assert G.edges == len(S.edges_of(n, rp, ci, va)[0])
    out = {}
    for sample in samples:
        comp, res = run(eng, G, n, sample)
        components, skipped, rounds, complete, kinds, hooks, jumps, edges, ns, total = res
        print(f"{name} sample={sample}: components {components} skipped {skipped} rounds {rounds} hooks {hooks.tolist()} "
              f"jumps {jumps.tolist()} edges {edges.tolist()} total_ns {total}")
        np.testing.assert_array_equal(comp, ref, err_msg=f"{name} sample={sample}")
        assert complete and components == int(np.count_nonzero(ref == np.arange(n)))
        assert 0 <= skipped <= largest and (sample > 0 or skipped == 0)
        assert len(kinds) == len(hooks) == len(jumps) == len(edges) == len(ns) == rounds > sample
        assert kinds.tolist() == [0] * sample + [1] * (rounds - sample)
        assert total >= int(ns.sum())
        out[sample] = res
    G.free()
    return out


def scc_comp(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.scc_graph(rp, ci, va)
    cv = eng.alloc(n).fill(7, np.int32)
    res = eng.scc(G, cv)
    comp = cv.download(np.int32, n=n)
    cv.free()
    G.free()
    assert res[5]
    return comp


# ------------------------------------------------------------------ 1. trivial inputs
def test_a_graph_without_rows(eng):
    G = eng.wcc_graph(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert G.edges == 0
    for sample in SAMPLES:
        comp, res = run(eng, G, 0, sample)
        assert len(comp) == 0 and res[:4] == (0, 0, 0, True) and all(len(a) == 0 for a in res[4:9]) and res[9] == 0
    G.free()


@pytest.mark.parametrize("name", ["empty", "loops"])
def test_every_vertex_alone(eng, name):
    n = matrix(name)[0]
    np.testing.assert_array_equal(want(name), np.arange(n))
    for res in check(eng, name).values():
        assert res[0] == n and int(res[5].sum()) == 0   # n components, no hook


def test_stored_zeros_and_columns_outside_join_nothing(eng):
    n, rp, ci, va = matrix("noise")
    assert (va == 0).sum() >= 4 * n and (ci == -1).any() and (ci == n).any() and (ci == n + 7).any()
    as_edges = W.components(n, rp, np.clip(ci, 0, n - 1), np.ones(len(ci), np.float32))
    assert np.count_nonzero(as_edges == np.arange(n)) < 100   # (if they counted, almost everything would hang together)
    check(eng, "noise")


# ------------------------------------------------------------------ 2. direction, hubs, list classes
@pytest.mark.parametrize("name", ["up", "down"])
def test_direction_is_ignored(eng, name):
    assert (want(name) == matrix(name)[0] - 1).all()
    check(eng, name)


@pytest.mark.parametrize("name", ["hub-out-largest", "hub-out-smallest", "hub-in-largest", "hub-in-smallest"])
def test_a_hub_of_70001_edges(eng, name):
    check(eng, name)


@pytest.mark.parametrize("name", ["limits-in", "limits-out"])
def test_list_lengths_at_the_class_limits(eng, name):
    assert np.count_nonzero(want(name) == np.arange(matrix(name)[0])) == len(W.CLASS_LENGTHS)
    check(eng, name)


def test_planted_components_with_noise(eng):
    check(eng, "planted")


# ------------------------------------------------------------------ 3. the path: rounds grow with log n, not with the diameter
@pytest.mark.parametrize("name", ["path-index", "path-reversed", "path-random"])
def test_a_path_of_65536_takes_few_rounds(eng, name):
    """A method bound by the diameter needs 65 535 rounds.  Jumping halves a chain's depth per sweep, so 16 sweeps undo the
    deepest chain one pass of hooks can build; four times that is allowed for the hooks in between: rounds <= 64."""
    n = matrix(name)[0]
    assert n == 65_536 and (want(name) == n - 1).all()
    for sample, res in check(eng, name).items():
        assert res[3] and res[2] <= 64, (name, sample, res[2])


# ------------------------------------------------------------------ 4. against sh_scc on symmetric patterns
def test_the_grid_is_one_component_and_equals_scc(eng):
    res = check(eng, "grid")
    assert (want("grid") == 128 * 128 - 1).all()
    np.testing.assert_array_equal(scc_comp(eng, "grid"), want("grid"))
    assert all(r[2] <= 64 for r in res.values())   # (diameter 254; not a bound of the issue's, but the point of the feature)


@pytest.mark.parametrize("name", ["rmat12", "rmat15"])
def test_symmetrised_rmat_equals_scc_and_skips_the_giant(eng, name):
    res = check(eng, name)
    np.testing.assert_array_equal(scc_comp(eng, name), want(name))
    assert res[2][1] > 0                       # sample = 2: the giant component's lists are not walked
    assert res[2][7].sum() < res[0][7].sum()   # ... and fewer entries are looked at than without sampling


def test_rmat_as_generated(eng):
    n, rp, ci, va = matrix("rmat15-directed")
    np.testing.assert_array_equal(want("rmat15-directed"), H.wcc_labels(rp, ci, va))
    check(eng, "rmat15-directed")


# ------------------------------------------------------------------ 5. the skip's two blind spots; no giant; a large sample
@pytest.mark.parametrize("name", ["pendants-out", "pendants-in"])
def test_edges_between_the_skipped_tree_and_the_rest(eng, name):
    """pendants-out: the tying edge is stored only in the giant member's row, so it is seen only through the pendant's
    out-list.  pendants-in: only in the pendant's row at position 6, so only through its in-list in a full round."""
    n = matrix(name)[0]
    assert (want(name) == n - 1).all()
    res = check(eng, name)
    assert res[2][1] >= 19_000   # sample = 2 found (most of) the giant, and it was skipped


def test_no_giant_at_all(eng):
    res = check(eng, "no-giant")
    assert all(r[0] == 12_000 and r[1] <= 2 for r in res.values())


def test_a_sample_larger_than_every_list(eng):
    n, rp, ci, va = matrix("grid")
    assert np.diff(rp).max() == 4
    res = check(eng, "grid", samples=(9,))[9]
    assert res[7][4:9].sum() == 0   # rounds 4 .. 8 found no entry to look at


# ------------------------------------------------------------------ 6. the round cap and the handle
def test_a_run_cut_short_leaves_no_partition_and_the_handle_stays_good(eng):
    n, rp, ci, va = matrix("path-random")
    G = eng.wcc_graph(rp, ci, va)
    for sample in (0, 2):
        comp, res = run(eng, G, n, sample, cap=1)
        assert not res[3] and res[2] == 1 and res[0] == 0 and (comp == -1).all()
        assert len(res[4]) == 1 and res[4][0] == (0 if sample else 1)
    first, res = run(eng, G, n)
    np.testing.assert_array_equal(first, want("path-random"))
    assert res[3]
    again, res = run(eng, G, n)
    np.testing.assert_array_equal(again, first)
    assert res[3]
    G.free()


def test_per_round_arrays(eng):
    res = check(eng, "pendants-out", samples=(2,))[2]
    components, skipped, rounds, complete, kinds, hooks, jumps, edges, ns, total = res
    assert kinds[:2].tolist() == [0, 0] and (kinds[2:] == 1).all() and rounds >= 4
    assert hooks[2:].sum() >= 500 and hooks[-1] == 0 and jumps[-1] == 0   # the pendants are hooked by full rounds
    assert edges[2] >= 500 and (ns > 0).all()


# ------------------------------------------------------------------ 7. footprint, comp's length
@pytest.mark.parametrize("name", ["empty", "limits-in", "hub-out-largest", "rmat12"])
def test_footprint_is_the_headers_formula(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.wcc_graph(rp, ci, va)
    rows, edges = n, G.edges
    assert edges == len(S.edges_of(n, rp, ci, va)[0])
    assert G.footprint == 8 * (rows + 1) + 8 * edges + 8 * rows + 16 * (edges // 1024 + 1) + 8 * (edges // 2048 + 1) + 34816
    G.free()


def test_comp_is_overwritten_in_full_and_not_beyond(eng):
    n, rp, ci, va = matrix("planted")
    G = eng.wcc_graph(rp, ci, va)
    cv = eng.alloc(n + 5).fill(7, np.int32)
    eng.wcc(G, cv)
    got = cv.download(np.int32)
    np.testing.assert_array_equal(got[:n], want("planted"))
    assert (got[n:] == 7).all()
    cv.free()
    short = eng.alloc(n - 1).fill(7, np.int32)
    with pytest.raises(EngineError, match="comp is shorter") as err:
        eng.wcc(G, short)
    assert err.value.code == abi.SH_ESHAPE
    assert (short.download(np.int32) == 7).all()   # reported before any device work
    short.free()
    G.free()
