"""sh_rcm on the GPU: perm, pos, level, the components, the searches, the steps, bandwidth and profile before and after,
and the record of every step against tests/rcm_ref.py (pinned by tests/test_rcm_ref.py) and, on the shapes Python cannot
afford, against the host gold (which tests/test_rcm_ref.py pins against the reference, records included).

Every comparison is exact (==): with the ties fixed by (deg, index) a graph has one answer, whatever the lanes race on.
The shapes are the smallest at which a kernel can still go wrong: lists on both sides of the walk's tiers (one lane up
to 8 entries, one wave up to 2048, the workgroup beyond) and of a wave's and a workgroup's chunk (64, 256), one position
with 70 001 children, a level wider than a launch has lanes (every workgroup's chunk and the scan of the totals), a level
whose every vertex is claimed by 70 positions, more steps than the first two batches hold, many components with ties."""
import ctypes as C

import numpy as np
import pytest

import core_ref as R
import guarded as GD
import msf_ref as M
import rcm_ref as X
import tri_ref as T
import wcc_ref as W
from guarded import _not_halted   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

STARS = (7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)   # either side of RCM_LANE, 64, WL_BS and RCM_WAVE
MAKERS = {
    "one-row": lambda: X.empty(1),
    "lonely": lambda: X.empty(300),
    "graphs4": X.all_graphs4,
    "path": lambda: W.path(100, order="index"),
    "stars": lambda: X.stars(STARS),
    "K70,70": lambda: T.bipartite(70, 70),
    "islands": lambda: M.islands(),
    "hub": R.big_hub,
    "broom": X.broom,
    "grid400": lambda: X.shuffled(W.grid(400)),
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
}
_cache, _want = {}, {}


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


def want(name, sweeps=8, reverse=1, max_steps=None, gold=False, mat=None):
    """The reference's answer and records (gold: the host's), computed once per case and left unchanged."""
    key = (name, sweeps, reverse, max_steps, gold)
    if key not in _want:
        mat = matrix(name) if mat is None else mat
        if gold:
            perm, pos, level, bw0, bw1, p0, p1, comps, searches, kinds, sizes, edges = H.rcm_order(
                *mat[1:], sweeps=sweeps, reverse=reverse, records=True)
            r = dict(perm=perm, pos=pos, level=level, components=comps, sweeps_run=searches, steps=len(kinds), complete=True,
                     kind=kinds, size=sizes, edges=edges, bandwidth_before=bw0, bandwidth_after=bw1, profile_before=p0,
                     profile_after=p1)
        else:
            r = X.levels(*mat, sweeps=sweeps, reverse=reverse, max_steps=max_steps)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = r
    return _want[key]


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_rcm_abi.py asserts that the header states it)."""
    return 4 * (n + 1) + 28 * n + 8 * edges + 50176


def run(eng, mat, sweeps=8, reverse=1, max_steps=None, G=None):
    """-> dict of one call's outputs (on a handle of its own unless G is given)."""
    n = mat[0]
    own = G is None
    if own:
        G = eng.rcm_graph(*mat[1:])
    vecs = [eng.alloc(max(n, 1)) for _ in range(3)]
    try:
        for v in vecs:
            v.upload(np.full(max(n, 1), 7, np.int32))
        (components, sweeps_run, steps, complete, bw0, bw1, p0, p1, kinds, sizes, edges, ns, total) = eng.rcm_order(
            G, *vecs, sweeps=sweeps, reverse=reverse, max_steps=max_steps)
        perm, pos, level = (v.download(np.int32, n) if n else np.zeros(0, np.int32) for v in vecs)
        return dict(perm=perm, pos=pos, level=level, components=components, sweeps_run=sweeps_run, steps=steps,
                    complete=complete, kind=kinds, size=sizes, edges=edges, bandwidth_before=bw0, bandwidth_after=bw1,
                    profile_before=p0, profile_after=p1, M=G.edges, max_degree=G.max_degree, footprint=G.footprint, ns=ns)
    finally:
        for v in vecs:
            v.free()
        if own:
            G.free()


def same(got, w, n):
    for f in ("perm", "pos", "level", "kind", "size", "edges"):
        assert np.array_equal(got[f], w[f]), f
    for f in ("components", "sweeps_run", "steps", "bandwidth_before", "bandwidth_after", "profile_before", "profile_after"):
        assert got[f] == w[f], (f, got[f], w[f])
    assert got["complete"] is w["complete"]
    assert len(got["ns"]) == got["steps"]
    if "M" in w:
        assert got["M"] == w["M"] and got["max_degree"] == w["max_degree"]
    assert got["footprint"] == header_footprint(n, got["M"])


def check(eng, name, sweeps=8, reverse=1, gold=False):
    mat = matrix(name)
    got = run(eng, mat, sweeps, reverse)
    same(got, want(name, sweeps, reverse, gold=gold), mat[0])
    assert got["complete"] is True and sorted(got["perm"].tolist()) == list(range(mat[0]))
    assert np.array_equal(got["perm"][got["pos"]], np.arange(mat[0]))
    return got


# ---- 1. nothing to order
def test_no_rows(eng):
    got = run(eng, X.empty(0))
    assert (got["components"], got["sweeps_run"], got["steps"], got["complete"], got["M"]) == (0, 0, 0, True, 0)
    assert (got["bandwidth_before"], got["bandwidth_after"], got["profile_before"], got["profile_after"]) == (0, 0, 0, 0)
    assert got["footprint"] == header_footprint(0, 0)


@pytest.mark.parametrize("name", ["one-row", "lonely"])
@pytest.mark.parametrize("reverse", [0, 1])
def test_vertices_without_an_edge_take_no_step(eng, name, reverse):
    got = check(eng, name, 8, reverse)
    n = matrix(name)[0]
    assert got["steps"] == 0 and got["components"] == n and (got["level"] == 0).all()
    assert got["perm"].tolist() == (list(range(n))[::-1] if reverse else list(range(n)))


# ---- 2. many components, ties, roots that move; the parameters
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("sweeps", [0, 1, 8])
def test_all_graphs_on_4_vertices_in_one_handle(eng, sweeps, reverse):
    got = check(eng, "graphs4", sweeps, reverse)
    assert got["components"] == want("graphs4", sweeps, reverse)["components"] == 98
    assert (got["sweeps_run"] == 0) == (sweeps == 0)


@pytest.mark.parametrize("sweeps", [0, 8])
def test_islands(eng, sweeps):
    check(eng, "islands", sweeps)


# ---- 3. more steps than the first two batches hold
def test_a_path_passes_the_batch_seams(eng):
    got = check(eng, "path")
    assert got["steps"] == 300 > sum(X.BATCHES[:2]) and (got["size"] == 1).all()
    assert got["kind"].tolist() == [0] * 200 + [1] * 100 and got["sweeps_run"] == 2
    # (the search from 99 is no longer than the one from 0: 0 stays the root, and the order is reversed)
    assert got["bandwidth_after"] == 1 and got["perm"].tolist() == list(range(100))[::-1]


# ---- 4. the list-walk tiers and their seams
def test_stars_on_either_side_of_every_tier(eng):
    got = check(eng, "stars")
    assert got["max_degree"] == max(STARS) and got["components"] == len(STARS) + 1
    check(eng, "stars", sweeps=0, reverse=0)


def test_hub_of_70001_leaves(eng):
    got = check(eng, "hub", gold=True)
    assert got["max_degree"] == 70_001 and got["bandwidth_after"] == 70_000   # a leaf is the root: the hub stands second


def test_broom_is_wider_than_a_launch(eng):
    got = check(eng, "broom", gold=True)
    # (every search starts at a pendant: itself, its leaf, the hub, the other 300 000 leaves, their pendants)
    assert got["max_degree"] == 300_001 and got["components"] == 1
    assert got["size"].tolist() == [1, 1, 1, 300_000, 300_000] * 3 and 300_000 > 1024 * 256


def test_every_vertex_of_a_level_claimed_by_70_positions(eng):
    got = check(eng, "K70,70")
    assert got["size"][got["kind"] == 1].tolist() == [1, 70, 69]
    check(eng, "K70,70", sweeps=0)


# ---- 5. larger graphs against the host gold
def test_shuffled_grid(eng):
    got = check(eng, "grid400", gold=True)
    assert got["bandwidth_after"] <= got["bandwidth_before"] and got["bandwidth_after"] == 400
    assert got["profile_after"] < got["profile_before"]


@pytest.mark.parametrize("sweeps", [0, 8])
def test_rmat12(eng, sweeps):
    check(eng, "rmat12", sweeps, gold=True)


# ---- 6. one handle, several calls; two handles
def test_two_calls_on_one_handle_with_different_sweeps(eng):
    """Stamps, owner and cnt must not carry over from call to call."""
    mat = matrix("graphs4")
    G = eng.rcm_graph(*mat[1:])
    try:
        for sweeps, reverse in ((8, 1), (0, 1), (8, 1), (1, 0)):
            same(run(eng, mat, sweeps, reverse, G=G), want("graphs4", sweeps, reverse), mat[0])
    finally:
        G.free()


def test_two_handles_interleaved(eng):
    a, b = matrix("islands"), matrix("stars")
    Ga, Gb = eng.rcm_graph(*a[1:]), eng.rcm_graph(*b[1:])
    try:
        for sweeps in (8, 0, 8):
            ga = run(eng, a, sweeps, G=Ga)
            gb = run(eng, b, sweeps, G=Gb)
            same(ga, want("islands", sweeps), a[0])
            same(gb, want("stars", sweeps), b[0])
    finally:
        Ga.free()
        Gb.free()


# ---- 7. max_steps cuts a run short; the handle serves the next call
@pytest.mark.parametrize("name,cap", [("path", 50), ("path", 250), ("graphs4", 37), ("graphs4", 200), ("stars", 3)])
def test_cut_short_and_reuse(eng, name, cap):
    """path: 50 steps end in the middle of the first search, 250 in the middle of the numbering."""
    mat = matrix(name)
    n = mat[0]
    full, part = want(name), want(name, max_steps=cap)
    assert part["complete"] is False and part["steps"] == cap
    G = eng.rcm_graph(*mat[1:])
    try:
        got = run(eng, mat, max_steps=cap, G=G)
        same(got, part, n)
        there = got["perm"] >= 0
        assert there.sum() == part["done"] and np.array_equal(got["perm"][there], full["perm"][there])
        assert (got["bandwidth_after"], got["profile_after"]) == (-1, -1)
        same(run(eng, mat, G=G), full, n)
    finally:
        G.free()
    if name == "path":
        assert part["done"] == (0 if cap == 50 else 51) and part["kind"][-1] == (0 if cap == 50 else 1)


# ---- 8. the call's face
def test_refusals_and_operands_only(eng):
    """pos, level and every per-step array NULL; vectors longer than rows keep their tails and their guard words; short
    ones and bad scalars are refused with the buffers untouched."""
    mat = matrix("islands")
    n = mat[0]
    w = want("islands")
    lib = abi.load()
    dev = GD.Dev(lib, eng.h)
    G = eng.rcm_graph(*mat[1:])
    spare = 5
    vecs = [dev.guarded(np.full(n + spare, 7, np.int32), offset=k) for k in range(3)]
    short = dev.guarded(np.full(n - 1, 7, np.int32))
    try:
        i32 = [C.c_int32() for _ in range(4)]
        i64 = [C.c_int64() for _ in range(4)]
        rc = lib.sh_rcm(eng.h, G.h, vecs[0].h, None, None, 8, 1, 10_000, *[C.byref(x) for x in i32 + i64], *(None,) * 5)
        assert rc == abi.SH_OK
        assert [x.value for x in i32] == [w["components"], w["sweeps_run"], w["steps"], 1]
        assert [x.value for x in i64] == [w["bandwidth_before"], w["bandwidth_after"], w["profile_before"], w["profile_after"]]
        p = vecs[0].read("perm").view(np.int32)
        assert np.array_equal(p[:n], w["perm"]) and (p[n:] == 7).all()
        for v in vecs[1:]:
            assert (v.read("not passed").view(np.int32) == 7).all()
        eng.rcm_order(G, *vecs)
        for v, f in zip(vecs, ("perm", "pos", "level")):
            got = v.read(f).view(np.int32)
            assert np.array_equal(got[:n], w[f]) and (got[n:] == 7).all(), f
        for v in vecs:
            dev.ok(lib.sh_vec_upload(eng.h, v.v, GD.vp(np.full(n + spare, 7, np.int32)), n + spare))
        for bad in ((short, None, None), (vecs[0], short, None), (vecs[0], vecs[1], short)):
            with pytest.raises(EngineError) as err:
                eng.rcm_order(G, *bad)
            assert err.value.code == abi.SH_ESHAPE
        for bad in (dict(sweeps=-1), dict(sweeps=65), dict(reverse=2), dict(reverse=-1), dict(max_steps=0), dict(max_steps=-3)):
            with pytest.raises(EngineError) as err:
                eng.rcm_order(G, *vecs, **bad)
            assert err.value.code == abi.SH_EINVAL
        for v in vecs + [short]:
            assert (v.read("refused").view(np.int32) == 7).all()   # the buffers are untouched
    finally:
        for v in vecs + [short]:
            v.free()
        G.free()
