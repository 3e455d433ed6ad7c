"""sh_msf on the GPU: in_msf, comp, the ends and weights of the edges, the counts and the records of every round against
tests/msf_ref.py (pinned by tests/test_msf_ref.py), comp against tests/wcc_ref.py as well, and one larger case against
the host gold.

Every comparison is exact (==): no two keys are equal, so a matrix has one forest, whatever the lanes race on, and find
sees one state, so rounds, walked, kept and hooks are functions of the input.  The shapes are the smallest at which the
kernels can still go wrong: every graph on 4 vertices, ties everywhere (the 64 x 64 grid of equal weights: chains), more
rounds than the first batch holds (the ruler path), one chain of depth 70 000 in either hooking direction (the star
guarantee of the jump sweeps), one word wanted by 70 001 edges (the hub)."""
import ctypes as C

import numpy as np
import pytest

import msf_ref as F
import wcc_ref as W
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

_cache, _want = {}, {}


def _specials():
    """An 8 x 8 grid whose entries cycle through -NaN, -inf, a negative denormal, -0.0, the smallest denormal, +inf, +NaN,
    -1, 1e-38 and 3: NaNs of both signs, infinities, -0.0 and denormals as weights, the two directions of an edge mostly
    with different values."""
    bits = np.array([0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0x00000001, 0x7F800000, 0x7FC00000, 0xBF800000,
                     0x006CE3EE, 0x40400000, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800001], np.uint32)
    n, rp, ci, _ = W.grid(8)
    return n, rp, ci, np.resize(bits, len(ci)).view(np.float32)


def _parallel():
    """Parallel entries and the two directions of an edge with different values, among noise: the smaller wins."""
    rp = np.array([0, 3, 8, 10, 10], np.int32)
    ci = np.array([1, 0, 1, 0, 0, 2, 9, 1, 1, 3], np.int32)
    va = np.array([5, 9, 4, 2, 3, -1, 1, 0, 7, -0.0], np.float32)
    return 4, rp, ci, va


MAKERS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "one-row": lambda: (1, np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "no-edges": lambda: (300, np.zeros(301, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "noise": F.noise,
    "parallel": _parallel,
    "specials": _specials,
    "grid64-unit": lambda: F.weighted(W.grid(64), "unit"),
    "ruler": lambda: F.ruler_path(1024),
    "chain-up": lambda: F.chain_path(70_001, True),
    "chain-down": lambda: F.chain_path(70_001, False),
    "hub": lambda: F.hub(70_001),
    "rmat12-drawn": lambda: F.weighted((1 << 12,) + H.rmat(12, seed=40), "drawn", seed=8),
    "rmat12-unit": lambda: F.weighted((1 << 12,) + H.rmat(12, seed=40), "unit"),
    "grid128-drawn": lambda: F.weighted(W.grid(128), "drawn", seed=9),
    "islands": F.islands,
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


def want(name, max_rounds=33, mat=None):
    """The reference's answer and records, computed once per pattern and left unchanged."""
    key = (name, max_rounds)
    if key not in _want:
        mat = matrix(name) if mat is None else mat
        r = F.schedule(*mat, max_rounds=max_rounds)
        if r["complete"]:
            n = mat[0]
            assert np.array_equal(r["in_msf"], F.kruskal(n, r["eu"], r["ev"], F.order_key(r["weight"])))
            assert np.array_equal(r["comp"], W.components(*mat) if n else np.zeros(0, np.int32))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = r
    return _want[key]


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_msf_abi.py asserts that the header states it)."""
    return 16 * n + 20 * edges + 33792


def run(eng, mat, max_rounds=33, G=None):
    """-> dict of one call's outputs (on a handle of its own unless G is given), every optional output asked for."""
    n = mat[0]
    own = G is None
    if own:
        G = eng.msf_graph(*mat[1:])
    M = G.edges
    vecs = [eng.alloc(max(k, 1)) for k in (M, n, M, M, M)]
    try:
        for v, k in zip(vecs, (M, n, M, M, M)):
            v.upload(np.full(max(k, 1), 7, np.int32))
        mv, cv, uv, vv, wv = vecs
        tree, comps, rounds, complete, walked, kept, hooks, jumps, ns, total = eng.spanning_forest(
            G, mv, comp=cv, edge_u=uv, edge_v=vv, weight=wv, max_rounds=max_rounds)
        get = lambda v, k, dt=np.int32: v.download(dt, k) if k else np.zeros(0, dt)   # noqa: E731
        return dict(in_msf=get(mv, M), comp=get(cv, n), eu=get(uv, M), ev=get(vv, M), weight=get(wv, M, np.uint32),
                    tree_edges=tree, components=comps, rounds=rounds, complete=complete, walked=walked, kept=kept,
                    hooks=hooks, jumps=jumps, M=M, footprint=G.footprint)
    finally:
        for v in vecs:
            v.free()
        if own:
            G.free()


def same(got, w, n):
    assert got["M"] == w["M"] and np.array_equal(got["eu"], w["eu"]) and np.array_equal(got["ev"], w["ev"])
    assert np.array_equal(got["weight"], w["weight"])
    assert np.array_equal(got["in_msf"], w["in_msf"])
    assert np.array_equal(got["comp"], w["comp"])
    assert got["complete"] is w["complete"] and got["rounds"] == w["rounds"]
    assert (got["tree_edges"], got["components"]) == (w["tree_edges"], w["components"])
    assert np.array_equal(got["walked"], w["walked"]) and np.array_equal(got["kept"], w["kept"])
    assert np.array_equal(got["hooks"], w["hooks"])
    assert got["footprint"] == header_footprint(n, w["M"])


def check(eng, name):
    mat = matrix(name)
    w = want(name)
    got = run(eng, mat)
    same(got, w, mat[0])
    assert got["complete"] is True and int(got["in_msf"].sum()) == got["tree_edges"] == mat[0] - got["components"]
    return got


# ---- 1. nothing to join
def test_no_rows(eng):
    got = run(eng, matrix("no-rows"))
    assert (got["tree_edges"], got["components"], got["rounds"], got["complete"], got["M"]) == (0, 0, 0, True, 0)
    assert got["footprint"] == header_footprint(0, 0)


@pytest.mark.parametrize("name", ["one-row", "no-edges", "noise"])
def test_no_edges(eng, name):
    got = check(eng, name)
    n = matrix(name)[0]
    assert got["M"] == 0 and got["rounds"] == 1 and got["components"] == n and got["comp"].tolist() == list(range(n))


# ---- 2. every graph on 4 labelled vertices, ties everywhere, ascending and descending in the edge id
@pytest.mark.parametrize("weights", ["equal", "ascending", "descending"])
def test_every_graph_on_four_vertices(eng, weights):
    for mask in range(64):
        mat = F.graph4(mask, weights)
        same(run(eng, mat), want(("graph4", mask, weights), mat=mat), 4)


# ---- 3. the weight rules
def test_parallel_entries_and_both_directions_the_smaller_wins(eng):
    got = check(eng, "parallel")
    assert got["eu"].tolist() == [0, 1, 2] and got["ev"].tolist() == [1, 2, 3]
    # {0, 1}: 5, 4, 2 and 3 stored, 2 wins; {1, 2}: -1 and 7; {2, 3}: a stored -0.0 is an edge (its bits are not all zero)
    assert got["weight"].tolist() == np.array([2.0, -1.0, -0.0], np.float32).view(np.uint32).tolist()
    assert got["in_msf"].tolist() == [1, 1, 1] and got["comp"].tolist() == [3, 3, 3, 3]


def test_special_values_have_their_place_in_the_order(eng):
    got = check(eng, "specials")
    k = F.order_key(got["weight"]).astype(np.int64)
    chosen = got["in_msf"] == 1
    assert int(chosen.sum()) == 63 and got["components"] == 1
    # a grid has no bridge, so the edge with the largest KEY closes a cycle of lighter edges and stays outside
    key = (k << 32) | np.arange(len(k))
    assert key[chosen].max() < key.max()
    # -NaN below -inf below the negative denormal below -0.0 below the smallest denormal below +inf below +NaN
    order = F.order_key(np.array([0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 1, 0x7F800000, 0x7FC00000], np.uint32))
    assert np.all(np.diff(order.astype(np.int64)) > 0)


# ---- 4. ties by edge id: one round, chains
def test_unit_weights_on_a_grid_build_chains_in_one_round(eng):
    got = check(eng, "grid64-unit")
    assert got["rounds"] == 2 and got["hooks"].tolist() == [4095, 0] and got["jumps"][0] > 0


# ---- 5. the ruler path: 11 rounds, over the first batch seam (8 rounds)
def test_ruler_path_crosses_the_first_batch_seam(eng):
    got = check(eng, "ruler")
    assert got["rounds"] == 11
    assert got["kept"].tolist() == [1023, 511, 255, 127, 63, 31, 15, 7, 3, 1, 0]
    assert got["hooks"].tolist() == [512, 256, 128, 64, 32, 16, 8, 4, 2, 1, 0]
    assert got["walked"].tolist() == [1023, 1023, 511, 255, 127, 63, 31, 15, 7, 3, 1]


# ---- 6. one chain of depth 70 000, hooked upwards and downwards: the star guarantee of the jump sweeps
@pytest.mark.parametrize("name", ["chain-up", "chain-down"])
def test_one_chain_of_depth_70000_is_a_star_after_the_round(eng, name):
    got = check(eng, name)
    assert got["rounds"] == 2 and got["hooks"].tolist() == [70_000, 0] and got["in_msf"].all()
    assert (got["comp"] == 70_000).all() and got["jumps"][0] >= 70_000 - 1


# ---- 7. one best word wanted by every edge
def test_hub_of_70001_leaves(eng):
    got = check(eng, "hub")
    assert got["rounds"] == 2 and got["in_msf"].all() and got["components"] == 1 and got["hooks"].tolist() == [70_001, 0]


# ---- 8. general patterns
@pytest.mark.parametrize("name", ["rmat12-drawn", "rmat12-unit", "grid128-drawn", "islands"])
def test_patterns(eng, name):
    got = check(eng, name)
    n = matrix(name)[0]
    assert got["rounds"] <= int(np.log2(n)) + 1
    if name == "islands":
        assert got["components"] == 4 + 11


# ---- 9. max_rounds cuts a run short; the handle serves the next call
def test_cut_short_and_reuse(eng):
    mat = matrix("ruler")
    full, part = want("ruler"), want("ruler", max_rounds=1)
    G = eng.msf_graph(*mat[1:])
    try:
        got = run(eng, mat, max_rounds=1, G=G)
        same(got, part, mat[0])
        assert got["complete"] is False and got["rounds"] == 1 and (got["comp"] == -1).all()
        assert got["in_msf"][0::2].all() and not got["in_msf"][1::2].any() and got["tree_edges"] == 512
        same(run(eng, mat, G=G), full, mat[0])
    finally:
        G.free()


# ---- 10. two handles, calls alternated
def test_two_handles_interleaved(eng):
    a, b = matrix("rmat12-drawn"), matrix("islands")
    Ga, Gb = eng.msf_graph(*a[1:]), eng.msf_graph(*b[1:])
    try:
        for _ in range(3):
            ga = run(eng, a, G=Ga)
            gb = run(eng, b, G=Gb)
            same(ga, want("rmat12-drawn"), a[0])
            same(gb, want("islands"), b[0])
    finally:
        Ga.free()
        Gb.free()


# ---- 11. the call's face
def test_optional_outputs_through_the_abi(eng):
    """Every optional output NULL; vectors longer than needed keep their tails; short ones and a bad scalar are refused
    with the buffers untouched."""
    n, rp, ci, va = matrix("rmat12-drawn")
    w = want("rmat12-drawn")
    M = w["M"]
    lib = abi.load()
    G = eng.msf_graph(rp, ci, va)
    spare = 5
    mv, cv, uv, vv, wv = (eng.alloc(k + spare) for k in (M, n, M, M, M))
    short_m, short_c = eng.alloc(M - 1), eng.alloc(n - 1)
    try:
        for v in (mv, cv, uv, vv, wv, short_m, short_c):
            v.upload(np.full(len(v), 7, np.int32))
        te, cc, rd, cp = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        rc = lib.sh_msf(eng.h, G.h, mv.h, None, None, None, None, 33, C.byref(te), C.byref(cc), C.byref(rd), C.byref(cp),
                        None, None, None, None, None, None)
        assert rc == abi.SH_OK
        assert (te.value, cc.value, rd.value, cp.value) == (w["tree_edges"], w["components"], w["rounds"], 1)
        m = mv.download(np.int32)
        assert np.array_equal(m[:M], w["in_msf"]) and (m[M:] == 7).all()
        for v in (cv, uv, vv, wv):
            assert (v.download(np.int32) == 7).all()                     # what was not asked for is not written
        eng.spanning_forest(G, mv, comp=cv, edge_u=uv, edge_v=vv, weight=wv)
        for v, k, ref in ((mv, M, w["in_msf"]), (cv, n, w["comp"]), (uv, M, w["eu"]), (vv, M, w["ev"]),
                          (wv, M, w["weight"].view(np.int32))):
            got = v.download(np.int32)
            assert np.array_equal(got[:k], ref) and (got[k:] == 7).all()   # the tails stay
        mv.upload(np.full(M + spare, 7, np.int32))
        cv.upload(np.full(n + spare, 7, np.int32))
        for bad in (dict(in_msf=short_m), dict(comp=short_c), dict(edge_u=short_m), dict(edge_v=short_m), dict(weight=short_m)):
            args = dict(in_msf=mv, comp=cv)
            args.update(bad)
            with pytest.raises(EngineError) as err:
                eng.spanning_forest(G, args.pop("in_msf"), **args)
            assert err.value.code == abi.SH_ESHAPE
        with pytest.raises(EngineError) as err:
            eng.spanning_forest(G, mv, comp=cv, max_rounds=0)
        assert err.value.code == abi.SH_EINVAL
        for v in (mv, cv, short_m, short_c):
            assert (v.download(np.int32) == 7).all()                     # the buffers are untouched
    finally:
        for v in (mv, cv, uv, vv, wv, short_m, short_c):
            v.free()
        G.free()


# ---- 12. against the host gold
def test_rmat15_against_the_host_gold(eng):
    rp, ci, _ = H.rmat(15, seed=40)
    mat = F.weighted((1 << 15, rp, ci, None), "drawn", seed=10)
    eu, ev, weight, in_msf, comp, M, components = H.msf_edges(*mat[1:])
    got = run(eng, mat)
    assert got["M"] == M and np.array_equal(got["eu"], eu) and np.array_equal(got["ev"], ev)
    assert np.array_equal(got["weight"], weight) and np.array_equal(got["in_msf"], in_msf)
    assert np.array_equal(got["comp"], comp) and got["components"] == components and got["complete"] is True
    assert got["tree_edges"] == int(in_msf.sum()) and got["rounds"] <= 16
    assert got["walked"][0] == M and np.array_equal(got["walked"][1:], got["kept"][:-1]) and got["kept"][-1] == 0
