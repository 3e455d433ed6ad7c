"""sh_match on the GPU: mate, in_match, the ends and weights of the edges, pairs, rounds, complete and the records of
every round against tests/match_ref.py (pinned by tests/test_match_ref.py); the larger inputs against the host gold for
mate / in_match, against certify() -- which needs no gold -- and against the simulator's rounds.

Every comparison is exact (==): no two keys are equal, so a matrix has one greedy matching under an order, whatever the
lanes race on, and bid sees one state, so rounds, walked, kept and matched are functions of the input, heavy and seed.
The shapes are the smallest at which the kernels can still go wrong: every graph on 4 vertices in one handle, list
lengths on either side of a wave's and a workgroup's seams, more rounds than the first two batches hold (the ascending
path), more edges than a full launch has lanes (the 400 x 400 grid), one word wanted by 70 001 edges (the hub)."""
import ctypes as C

import numpy as np
import pytest

import match_ref as M
import msf_ref as F
import wcc_ref as W
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

_cache, _want = {}, {}
ORDERS = [(heavy, seed) for heavy in (0, 1) for seed in (0, 7)]


def _specials():
    """An 8 x 8 grid whose entries cycle through NaNs of both signs, infinities, -0.0 and denormals (tests/test_msf_gpu.py's
    table), the two directions of an edge mostly with different values."""
    bits = np.array([0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0x00000001, 0x7F800000, 0x7FC00000, 0xBF800000,
                     0x006CE3EE, 0x40400000, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800001], np.uint32)
    n, rp, ci, _ = W.grid(8)
    return n, rp, ci, np.resize(bits, len(ci)).view(np.float32)


def _special_star():
    """A hub (vertex 0) with one leaf per special value, both directions stored with the same bits, and leaf 8 tied in
    by a stored +0.0 (no edge): whom the hub is matched with is the first (heavy == 0) or last (heavy == 1) of the order
    -NaN < -inf < -1 < negative denormal < -0.0 < denormal < 1 < +inf < +NaN."""
    bits = np.array([0x00000001, 0x7F800000, 0x80000000, 0xFFC00000, 0x3F800000, 0x7FC00000, 0xFF800000, 0x00000000,
                     0x80000001, 0xBF800000], np.uint32)
    k = len(bits)
    leaf = np.arange(1, k + 1, dtype=np.int64)
    hubs = np.zeros(k, np.int64)
    return W.csr(k + 1, np.concatenate([hubs, leaf]), np.concatenate([leaf, hubs]), np.concatenate([bits, bits]).view(np.float32))


def _parallel():
    """Parallel entries and the two directions of an edge with different values, among noise (tests/test_msf_gpu.py's):
    the smaller by k is the weight."""
    rp = np.array([0, 3, 8, 10, 10], np.int32)
    ci = np.array([1, 0, 1, 0, 0, 2, 9, 1, 1, 3], np.int32)
    va = np.array([5, 9, 4, 2, 3, -1, 1, 0, 7, -0.0], np.float32)
    return 4, rp, ci, va


MAKERS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "one-row": lambda: (1, np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "no-entries": lambda: (300, np.zeros(301, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "noise": F.noise,
    "parallel": _parallel,
    "specials": _specials,
    "special-star": _special_star,
    "path-60": lambda: M.ascending_path(60),
    "grid400-unit": lambda: F.weighted(W.grid(400), "unit"),
    "hub": lambda: M.hub(70_001),
    "rmat12-drawn": lambda: F.weighted((1 << 12,) + H.rmat(12, seed=40), "drawn", seed=8),
    "rmat12-unit": lambda: F.weighted((1 << 12,) + H.rmat(12, seed=40), "unit"),
    "islands": F.islands,
}
for _w in ("equal", "ascending", "descending"):
    MAKERS["packed4-" + _w] = lambda _w=_w: M.packed4(_w)
for _m in (63, 64, 65, 255, 256, 257):
    MAKERS[f"stars-{_m}"] = lambda _m=_m: M.stars_and_path(_m)


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


def want(name, heavy, seed, max_rounds=1 << 30, mat=None):
    """The reference's answer and records, computed once per pattern and order and left unchanged."""
    key = (name, heavy, seed, max_rounds)
    if key not in _want:
        n, eu, ev, weight, keys = M.case(matrix(name) if mat is None else mat, heavy, seed)
        r = M.rounds(n, eu, ev, keys, max_rounds=max_rounds)
        r.update(eu=eu, ev=ev, weight=weight, keys=keys, M=len(eu))
        if r["complete"]:
            assert M.certify(r["mate"], eu, ev, keys) == ""
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = r
    return _want[key]


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_match_abi.py parses the header's and compares)."""
    return 8 * n + 20 * edges + 17408


def run(eng, mat, heavy=1, seed=1, max_rounds=4096, G=None):
    """-> dict of one call's outputs (on a handle of its own unless G is given), every optional output asked for."""
    n = mat[0]
    own = G is None
    if own:
        G = eng.match_graph(*mat[1:])
    m = G.edges
    sizes = (n, m, m, m, m)
    vecs = [eng.alloc(max(k, 1)) for k in sizes]
    try:
        for v in vecs:
            v.fill(7, np.int32)
        tv, iv, uv, vv, wv = vecs
        pairs, rounds, complete, walked, kept, matched, ns, total = eng.matching(
            G, tv, heavy=heavy, seed=seed, in_match=iv, edge_u=uv, edge_v=vv, weight=wv, max_rounds=max_rounds)
        get = lambda v, k, dt=np.int32: v.download(dt, k) if k else np.zeros(0, dt)   # noqa: E731
        return dict(mate=get(tv, n), in_match=get(iv, m), eu=get(uv, m), ev=get(vv, m), weight=get(wv, m, np.uint32),
                    pairs=pairs, rounds=rounds, complete=complete, walked=walked, kept=kept, matched=matched, M=m,
                    footprint=G.footprint)
    finally:
        for v in vecs:
            v.free()
        if own:
            G.free()


def same(got, w, n):
    assert got["M"] == w["M"] and np.array_equal(got["eu"], w["eu"]) and np.array_equal(got["ev"], w["ev"])
    assert np.array_equal(got["weight"], w["weight"])
    assert np.array_equal(got["mate"], w["mate"])
    assert np.array_equal(got["in_match"], w["in_match"])
    assert got["complete"] is w["complete"] and got["rounds"] == w["rounds"] and got["pairs"] == w["pairs"]
    assert np.array_equal(got["walked"], w["walked"]) and np.array_equal(got["kept"], w["kept"])
    assert np.array_equal(got["matched"], w["matched"])
    assert got["footprint"] == header_footprint(n, w["M"])


def check(eng, name, heavy=1, seed=1, G=None):
    mat = matrix(name)
    w = want(name, heavy, seed)
    got = run(eng, mat, heavy, seed, G=G)
    same(got, w, mat[0])
    assert got["complete"] is True and int(got["in_match"].sum()) == got["pairs"] == int((got["mate"] >= 0).sum()) // 2
    return got


def check_all_orders(eng, name):
    """One handle, every order: (heavy, seed) is a property of the call."""
    G = eng.match_graph(*matrix(name)[1:])
    try:
        return {o: check(eng, name, *o, G=G) for o in ORDERS}
    finally:
        G.free()


# ---- 1. nothing to match
def test_no_rows(eng):
    got = run(eng, matrix("no-rows"))
    assert (got["pairs"], got["rounds"], got["complete"], got["M"]) == (0, 0, True, 0)
    assert got["footprint"] == header_footprint(0, 0)


@pytest.mark.parametrize("name", ["one-row", "no-entries", "noise"])
def test_rows_but_no_edges(eng, name):
    got = check(eng, name)
    n = matrix(name)[0]
    assert got["M"] == 0 and got["rounds"] == 1 and got["pairs"] == 0 and got["mate"].tolist() == [-1] * n
    assert got["walked"].tolist() == [0] and got["kept"].tolist() == [0] and got["matched"].tolist() == [0]


# ---- 2. every graph on 4 labelled vertices, block-diagonally in one handle per weight scheme
@pytest.mark.parametrize("weights", ["equal", "ascending", "descending"])
def test_every_graph_on_four_vertices(eng, weights):
    got = check_all_orders(eng, "packed4-" + weights)
    for g in got.values():
        assert np.all((g["mate"] < 0) | (g["mate"] // 4 == np.arange(256) // 4))   # nobody leaves its graph
    if weights == "equal":   # the seed decides among equal weights, heavy then decides nothing
        assert not np.array_equal(got[(0, 0)]["mate"], got[(0, 7)]["mate"])
        assert np.array_equal(got[(0, 7)]["mate"], got[(1, 7)]["mate"])
    else:                    # the weights differ: heavy decides, the seed nothing
        assert not np.array_equal(got[(0, 0)]["mate"], got[(1, 0)]["mate"])
        assert np.array_equal(got[(0, 0)]["mate"], got[(0, 7)]["mate"])


# ---- 3. the weight rules
def test_parallel_entries_and_both_directions_the_smaller_wins(eng):
    got = check(eng, "parallel", heavy=0, seed=0)
    assert got["eu"].tolist() == [0, 1, 2] and got["ev"].tolist() == [1, 2, 3]
    # {0, 1}: 5, 4, 2 and 3 stored, 2 wins; {1, 2}: -1 and 7; {2, 3}: a stored -0.0 is an edge (its bits are not all zero)
    assert got["weight"].tolist() == np.array([2.0, -1.0, -0.0], np.float32).view(np.uint32).tolist()
    assert got["mate"].tolist() == [-1, 2, 1, -1]        # lightest first: -1 < -0.0 < 2
    got = check(eng, "parallel", heavy=1, seed=0)
    assert got["mate"].tolist() == [1, 0, 3, 2]          # heaviest first: 2, then -0.0


def test_special_values_each_change_who_is_matched(eng):
    """The hub's leaves in the order of their weights; leaf 8 hangs on a stored +0.0, which is no edge.  Taking away
    the hub's partner, lightest or heaviest first, hands the hub to the next of the order: every special value has its
    place, and each of them changes who is matched."""
    n, rp, ci, va = matrix("special-star")
    order = [4, 7, 10, 9, 3, 1, 5, 2, 6]   # -NaN, -inf, -1, negative denormal, -0.0, denormal, 1, +inf, +NaN
    for heavy in (0, 1):
        left = list(order if heavy == 0 else order[::-1])
        vals = va.copy()
        while left:
            got = run(eng, (n, rp, ci, vals), heavy=heavy, seed=0)
            assert got["M"] == len(left) and got["pairs"] == 1 and got["rounds"] == 2
            assert got["mate"][0] == left[0] and got["mate"][left[0]] == 0 and got["mate"][8] == -1
            row = np.repeat(np.arange(n), np.diff(rp))
            vals[((row == 0) & (ci == left[0])) | ((row == left[0]) & (ci == 0))] = 0.0   # the edge becomes a stored zero
            left.pop(0)
    check_all_orders(eng, "specials")


# ---- 4. list lengths on either side of a wave's and a workgroup's seams
@pytest.mark.parametrize("edges", [63, 64, 65, 255, 256, 257])
def test_list_lengths_at_the_seams_of_the_append(eng, edges):
    got = check_all_orders(eng, f"stars-{edges}")
    for g in got.values():
        assert g["M"] == edges and g["walked"][0] == edges and g["kept"][0] == edges
        assert g["rounds"] >= 2 and g["kept"][1] < g["walked"][1]   # every star drops 8 edges after its first pair


# ---- 5. the ascending path: one pair per round, over the batch seams at 8 and 24 rounds
def test_ascending_path_crosses_the_batch_seams(eng):
    got = check(eng, "path-60", heavy=0, seed=0)
    assert got["rounds"] == 31 and got["matched"].tolist() == [1] * 30 + [0] and got["pairs"] == 30
    assert got["kept"].tolist() == list(range(59, 0, -2)) + [0]
    assert got["mate"].tolist() == [v ^ 1 for v in range(60)]


# ---- 6. max_rounds cuts a run short; the handle serves the next call
@pytest.mark.parametrize("cap", [8, 9, 31])
def test_cut_short_and_reuse(eng, cap):
    mat = matrix("path-60")
    full, part = want("path-60", 0, 0), want("path-60", 0, 0, max_rounds=cap)
    G = eng.match_graph(*mat[1:])
    try:
        got = run(eng, mat, 0, 0, max_rounds=cap, G=G)
        same(got, part, mat[0])
        assert got["complete"] is (cap == 31) and got["rounds"] == cap and got["pairs"] == min(cap, 30)
        on = got["mate"] >= 0
        assert np.array_equal(got["mate"][on], full["mate"][on]) and np.all(got["in_match"] <= full["in_match"])
        assert int(on.sum()) == 2 * got["pairs"]
        same(run(eng, mat, 0, 0, G=G), full, mat[0])
    finally:
        G.free()


# ---- 7. more edges than a full launch has lanes: the grid-stride loops iterate
def test_grid_400_unit_weights(eng):
    mat = matrix("grid400-unit")
    got = check(eng, "grid400-unit", heavy=1, seed=1)
    assert got["M"] == 319_200 > 1024 * 256
    geu, gev, gw, gin, gmate, gM, pairs = H.greedy_matching(*mat[1:], heavy=1, seed=1)
    assert gM == got["M"] and np.array_equal(got["mate"], gmate) and np.array_equal(got["in_match"], gin)
    assert got["pairs"] == pairs
    assert M.certify(got["mate"], got["eu"], got["ev"], want("grid400-unit", 1, 1)["keys"]) == ""


# ---- 8. one best word wanted by every edge
def test_hub_of_70001_leaves(eng):
    got = check(eng, "hub")
    assert got["rounds"] == 2 and got["pairs"] == 1 and got["matched"].tolist() == [1, 0]
    assert got["walked"].tolist() == [70_001, 70_001] and got["kept"].tolist() == [70_001, 0]
    w = want("hub", 1, 1)
    assert got["mate"][0] == 1 + int(np.argmin(w["keys"]))


# ---- 9. general patterns
@pytest.mark.parametrize("name", ["rmat12-drawn", "rmat12-unit"])
@pytest.mark.parametrize("heavy", [0, 1])
def test_rmat12(eng, name, heavy):
    mat = matrix(name)
    got = check(eng, name, heavy=heavy, seed=1)
    geu, gev, gw, gin, gmate, gM, pairs = H.greedy_matching(*mat[1:], heavy=heavy, seed=1)
    assert np.array_equal(got["mate"], gmate) and np.array_equal(got["in_match"], gin) and got["pairs"] == pairs
    assert M.certify(got["mate"], got["eu"], got["ev"], want(name, heavy, 1)["keys"]) == ""


def test_islands(eng):
    got = check_all_orders(eng, "islands")
    for g in got.values():   # grids of 81, 25 and 4 vertices, a triangle, 11 vertices alone: odd components leave one free
        assert int((g["mate"] < 0).sum()) >= 1 + 1 + 1 + 11 and g["pairs"] >= 2 + 1


# ---- 10. two handles, calls alternated, another order per call: nothing leaks from one call into the next
def test_two_handles_interleaved(eng):
    a, b = matrix("rmat12-unit"), matrix("islands")
    Ga, Gb = eng.match_graph(*a[1:]), eng.match_graph(*b[1:])
    try:
        for heavy, seed in ((1, 1), (0, 0), (1, 7), (0, 7), (1, 1)):
            same(run(eng, a, heavy, seed, G=Ga), want("rmat12-unit", heavy, seed), a[0])
            same(run(eng, b, 1 - heavy, seed ^ 7, G=Gb), want("islands", 1 - heavy, seed ^ 7), b[0])
    finally:
        Ga.free()
        Gb.free()


# ---- 11. the all-ones key: the one edge whose key equals "no bid" is still matched when it is dominant
def test_the_all_ones_key(eng):
    last = np.array([0x7FFFFFFF], np.uint32).view(np.float32)[0]
    mat = F.by_edge(W.path(4), np.array([1.0, last, 1.0], np.float32))
    seed = M.unmix32(0xFFFFFFFF) ^ 1
    n, eu, ev, weight, keys = M.case(mat, 0, seed)
    assert keys[1] == M.MAX
    got = run(eng, mat, heavy=0, seed=seed)
    assert got["mate"].tolist() == [1, 0, 3, 2] and got["in_match"].tolist() == [1, 0, 1]
    lone = (4,) + W.csr(4, np.array([1]), np.array([2]), np.array([last], np.float32))[1:]
    got = run(eng, lone, heavy=0, seed=M.unmix32(0xFFFFFFFF))
    assert got["mate"].tolist() == [-1, 2, 1, -1] and got["matched"].tolist() == [1, 0] and got["pairs"] == 1


# ---- 12. the call's face
def test_optional_outputs_through_the_abi(eng):
    """Each optional output NULL or present; vectors have a guard word behind them, and exactly rows or M elements are
    written; short vectors and bad scalars are refused with the buffers untouched."""
    n, rp, ci, va = matrix("rmat12-drawn")
    w = want("rmat12-drawn", 1, 1)
    m = w["M"]
    lib = abi.load()
    G = eng.match_graph(rp, ci, va)
    tv, iv, uv, vv, wv = (eng.alloc(k + 1) for k in (n, m, m, m, m))
    short_n, short_m = eng.alloc(n - 1), eng.alloc(m - 1)
    every = (tv, iv, uv, vv, wv, short_n, short_m)
    refs = (w["mate"], w["in_match"], w["eu"], w["ev"], w["weight"].view(np.int32))
    try:
        pr, rd, cp = C.c_int64(), C.c_int32(), C.c_int32()
        for present in range(16):   # bit i: optional output i is asked for
            for v in every:
                v.fill(7, np.int32)
            opt = [v.h if present >> i & 1 else None for i, v in enumerate((iv, uv, vv, wv))]
            rc = lib.sh_match(eng.h, G.h, tv.h, *opt, 1, 1, 4096, C.byref(pr), C.byref(rd), C.byref(cp), None, None, None,
                              None, None)
            assert rc == abi.SH_OK and (pr.value, rd.value, cp.value) == (w["pairs"], w["rounds"], 1)
            for i, (v, ref) in enumerate(zip((tv, iv, uv, vv, wv), refs)):
                got = v.download(np.int32)
                if i == 0 or present >> (i - 1) & 1:
                    assert np.array_equal(got[:-1], ref) and got[-1] == 7, i   # the guard word stays
                else:
                    assert (got == 7).all(), i                                # what was not asked for is not written
        for v in every:
            v.fill(7, np.int32)
        for bad in (dict(mate=short_n), dict(in_match=short_m), dict(edge_u=short_m), dict(edge_v=short_m), dict(weight=short_m)):
            args = dict(mate=tv, in_match=iv)
            args.update(bad)
            with pytest.raises(EngineError) as err:
                eng.matching(G, args.pop("mate"), **args)
            assert err.value.code == abi.SH_ESHAPE
        for bad in (dict(max_rounds=0), dict(heavy=2), dict(heavy=-1)):
            with pytest.raises(EngineError) as err:
                eng.matching(G, tv, in_match=iv, **bad)
            assert err.value.code == abi.SH_EINVAL
        for v in every:
            assert (v.download(np.int32) == 7).all()                         # the buffers are untouched
    finally:
        for v in every:
            v.free()
        G.free()
