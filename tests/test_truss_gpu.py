"""sh_truss on the GPU: truss, support, the ends of every edge, the number of edges and of triangles, max_truss, levels,
rounds and the records of every round (k, size, walked) against tests/truss_ref.py (pinned by tests/test_truss_ref.py),
against closed forms and against the host gold.

Every comparison is exact (==): truss numbers are integers and a graph has one vector of them, whatever the lanes race
on.  The shapes are the smallest at which the kernels can still go wrong: shorter lists on both sides of the classes'
limits (one lane up to 8 entries, one wave up to 2048, pieces of 2048 beyond), one item of 35 pieces that 140 000
current edges reach for in one launch, more rounds than a batch holds (the triangulated grid, R-MAT)."""
import ctypes as C

import numpy as np
import pytest

import core_ref as K
import tri_ref as T
import truss_ref as R
import wcc_ref as W
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

_cache, _want = {}, {}


def _loops():
    n = 1000
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)


MAKERS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "empty": lambda: (5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "loops": _loops,
    "path": lambda: W.path(4096),
    "K300,200": lambda: T.bipartite(300, 200),
    "pattern": T.pattern,
    "noise": lambda: T.with_noise(*T.pattern()),
    "upper": lambda: T.upper_only(*T.pattern()),
    "lower": lambda: T.lower_only(*T.pattern()),
    "pattern5": lambda: T.pattern(300, 6000, 5),
    "K9": lambda: T.complete(9),
    "K300": lambda: T.complete(300),
    "cliques": lambda: K.cliques(2, 12),
    "friendship": lambda: T.friendship(500),
    "tgrid": lambda: T.triangulated_grid(128),
    "k5_ear": R.k5_ear,
    "k5_ear2": R.k5_ear2,
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
    "rmat13": lambda: (1 << 13,) + H.rmat(13, seed=40),
}
NO_EDGES = ("no-rows", "empty", "loops")
NO_TRIANGLES = ("path", "K300,200")
PATTERNS = ("pattern", "pattern5", "K9", "K300", "cliques", "friendship", "tgrid", "k5_ear", "k5_ear2", "rmat12")
HUB_LENGTHS = (R.SHORT, R.SHORT + 1, R.PIECE, R.PIECE + 1, 2 * R.PIECE + 1)   # L + 1: the hub edge's shorter list


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def matrix(name, maker=None):
    if name not in _cache:
        n, rp, ci, va = (maker or MAKERS[name])()[:4]
        _cache[name] = (n, rp, ci, np.ascontiguousarray(va))
    return _cache[name]


def want(name):
    """The reference's answer and records, computed once per pattern and left unchanged."""
    if name not in _want:
        r = R.peel(*matrix(name))
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[name] = r
    return _want[name]


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_truss_abi.py asserts that the header states it)."""
    return 4 * (n + 1) + 4 * n + 40 * edges + 51200


def run(eng, mat, max_rounds=None, G=None, outputs=("support", "edge_u", "edge_v")):
    """-> dict of one call's outputs (on a handle of its own unless G is given)."""
    own = G is None
    if own:
        G = eng.truss_graph(*mat[1:])
    m = G.edges
    vecs = {k: eng.alloc(max(m, 1)) for k in ("truss",) + tuple(outputs)}
    try:
        for v in vecs.values():
            v.upload(np.full(max(m, 1), 7, np.int32))
        max_truss, levels, rounds, complete, triangles, ks, sizes, walked, ns, total = eng.truss_numbers(
            G, vecs["truss"], *(vecs.get(k) for k in ("support", "edge_u", "edge_v")), max_rounds=max_rounds)
        got = {k: (v.download(np.int32, m) if m else np.zeros(0, np.int32)) for k, v in vecs.items()}
        got.update(max_truss=max_truss, levels=levels, rounds=rounds, complete=complete, triangles=triangles, k=ks, size=sizes,
                   walked=walked, M=m, max_degree=G.max_degree, footprint=G.footprint)
        return got
    finally:
        for v in vecs.values():
            v.free()
        if own:
            G.free()


def same(got, w, records=True):
    """got == w in everything a complete call returns."""
    for f in ("truss", "support", "edge_u", "edge_v"):
        assert np.array_equal(got[f], w[f]), f
    for f in ("M", "triangles", "max_truss", "levels"):
        assert got[f] == w[f], f
    assert got["complete"] is True
    assert int(got["size"].sum()) == w["M"]
    if records:
        assert got["rounds"] == w["rounds"]
        for f in ("k", "size", "walked"):
            assert np.array_equal(got[f], w[f]), f


def check(eng, name, mat=None, w=None):
    w = want(name) if w is None else w
    mat = matrix(name) if mat is None else mat
    n = mat[0]
    got = run(eng, mat)
    same(got, w)
    deg = np.bincount(np.concatenate([w["edge_u"], w["edge_v"]]), minlength=max(n, 1))
    assert got["max_degree"] == (int(deg.max()) if w["M"] else 0)
    assert got["footprint"] == header_footprint(n, w["M"])
    return got


# ---- 1. trivial inputs
@pytest.mark.parametrize("name", NO_EDGES)
def test_nothing_to_peel(eng, name):
    got = check(eng, name)
    assert got["M"] == 0 and got["rounds"] == 0 and got["max_truss"] == 0 and got["levels"] == 0 and got["triangles"] == 0


@pytest.mark.parametrize("name", NO_TRIANGLES)
def test_no_triangles_is_truss_two_in_one_round(eng, name):
    got = check(eng, name)
    assert (got["truss"] == 2).all() and (got["support"] == 0).all()
    assert got["rounds"] == 1 and got["levels"] == 1 and got["max_truss"] == 2 and got["triangles"] == 0


# ---- 2. every pattern
@pytest.mark.parametrize("name", PATTERNS)
def test_patterns(eng, name):
    check(eng, name)


def test_closed_forms(eng):
    truss = lambda name: run(eng, matrix(name))["truss"]   # noqa: E731
    assert (truss("K9") == 9).all() and (truss("K300") == 300).all()
    assert (truss("friendship") == 3).all() and (truss("tgrid") == 3).all()
    got = run(eng, matrix("cliques"))
    assert got["levels"] == 11 and got["max_truss"] == 12 and got["rounds"] == 11
    assert sorted(np.unique(got["truss"]).tolist()) == list(range(2, 13))
    got = run(eng, matrix("tgrid"))
    assert got["rounds"] == 128 and got["levels"] == 1 and got["triangles"] == 2 * 127 * 127
    assert run(eng, matrix("pattern5"))["rounds"] == 35   # more than the first batch of 8 and than a batch of 32
    assert truss("k5_ear").tolist() == [5, 5, 5, 5, 3, 5, 5, 5, 3, 5, 5, 5]
    assert truss("k5_ear2").tolist() == [5, 5, 5, 5, 3, 5, 5, 5, 3, 3, 5, 5, 5, 3]


def test_against_the_host_gold(eng):
    n, rp, ci, va = matrix("rmat13")
    eu, ev, sup, truss, m = H.truss_numbers(rp, ci, va)
    got = run(eng, matrix("rmat13"))
    assert got["M"] == m == 102_079 and got["triangles"] == int(sup.sum()) // 3 == 1_181_355
    for f, w in (("truss", truss), ("support", sup), ("edge_u", eu), ("edge_v", ev)):
        assert np.array_equal(got[f], w), f
    assert got["max_truss"] == int(truss.max()) == 63 and got["levels"] == len(np.unique(truss)) == 54
    assert got["complete"] is True and got["rounds"] == 401 and int(got["size"].sum()) == m


# ---- 3. noise and storage forms change nothing
def test_noise_and_storage_forms_change_nothing(eng):
    for form in ("noise", "upper", "lower"):
        check(eng, "pattern", mat=matrix(form))


# ---- 4. class limits of the shorter list
@pytest.mark.parametrize("length", HUB_LENGTHS)
def test_class_limits_two_hubs(eng, length):
    L = length - 1
    name = f"two_hubs{L}"
    matrix(name, lambda: R.two_hubs(L))
    got = check(eng, name)
    assert got["M"] == 2 * L + 1 and got["max_degree"] == length
    assert got["support"][0] == L and (got["support"][1:] == 1).all()      # edge 0 is {0, 1}
    assert (got["truss"] == 3).all() and got["triangles"] == L
    assert got["size"].tolist() == [2 * L, 1] and got["k"].tolist() == [3, 3]
    assert got["walked"].tolist() == [2 * L * 2, length]


# ---- 5. long lists, small support, live triangles
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("L", [R.PIECE - 5, R.PIECE, R.PIECE + 1])   # the hubs' lists hold L + 5 entries
def test_long_lists_small_support(eng, L, where):
    name = f"hub_pair{L}{where}"
    n, rp, ci, va, (u, v, w) = R.hub_pair(L, where)
    matrix(name, lambda: (n, rp, ci, va))
    got = check(eng, name)
    ends = list(zip(got["edge_u"].tolist(), got["edge_v"].tolist()))
    e_uv = ends.index((min(u, v), max(u, v)))
    assert got["support"][e_uv] == 1 and got["truss"][e_uv] == 3
    assert got["max_degree"] == L + 5
    assert sorted(np.unique(got["truss"], return_counts=True)[1].tolist()) == sorted([2 * L, 1, 20])
    assert got["size"].tolist() == [2 * L, 1, 20] and got["k"].tolist() == [2, 3, 5]


# ---- 6. the decrement race: 140 000 current edges reach for one word in one launch, then one item of 35 pieces
def test_decrement_race_gives_one_answer(eng):
    L = 70_000
    mat = matrix("two_hubs70000", lambda: R.two_hubs(L))
    G = eng.truss_graph(*mat[1:])
    try:
        runs = [run(eng, mat, G=G) for _ in range(5)]
    finally:
        G.free()
    first = runs[0]
    assert first["M"] == 2 * L + 1 and first["support"][0] == L and (first["support"][1:] == 1).all()
    assert (first["truss"] == 3).all() and first["triangles"] == L and first["complete"] is True
    assert first["size"].tolist() == [2 * L, 1] and first["walked"].tolist() == [4 * L, L + 1]
    for other in runs[1:]:
        for f in ("truss", "support", "edge_u", "edge_v", "k", "size", "walked"):
            assert np.array_equal(first[f], other[f]), f
        assert (other["rounds"], other["levels"], other["max_truss"], other["triangles"]) == (2, 1, 3, L)


# ---- 7. max_rounds cuts a run short; the handle serves the next call
def test_cut_short_and_reuse(eng):
    mat = matrix("tgrid")
    full = want("tgrid")
    part = R.peel(*mat, max_rounds=10)
    assert part["complete"] is False and (part["truss"] == 0).any() and (part["truss"] == 3).any()
    G = eng.truss_graph(*mat[1:])
    try:
        got = run(eng, mat, max_rounds=10, G=G)
        assert got["complete"] is False and got["rounds"] == 10
        assert np.array_equal(got["truss"], part["truss"])                  # settled edges their truss, the others 0
        assert np.array_equal(got["support"], full["support"]) and got["triangles"] == full["triangles"]
        assert np.array_equal(got["size"], full["size"][:10]) and np.array_equal(got["k"], full["k"][:10])
        assert np.array_equal(got["walked"], full["walked"][:10])
        again = run(eng, mat, G=G)
        same(again, full)
        none = run(eng, mat, max_rounds=0, G=G)
        assert none["complete"] is False and none["rounds"] == 0 and (none["truss"] == 0).all()
        assert np.array_equal(none["support"], full["support"]) and none["triangles"] == full["triangles"]
        same(run(eng, mat, G=G), full)
    finally:
        G.free()


# ---- 8. two handles, calls alternated
def test_two_handles_interleaved(eng):
    a, b = matrix("rmat12"), matrix("pattern5")
    Ga, Gb = eng.truss_graph(*a[1:]), eng.truss_graph(*b[1:])
    try:
        for _ in range(2):
            ga = run(eng, a, G=Ga)
            gb = run(eng, b, G=Gb)
            same(ga, want("rmat12"))
            same(gb, want("pattern5"))
    finally:
        Ga.free()
        Gb.free()


# ---- 9. the call's face
def test_optional_outputs_through_the_abi(eng):
    """Every optional output NULL or given; vectors longer than M keep their tail; short ones are refused with the
    buffers untouched."""
    n, rp, ci, va = matrix("pattern5")
    w = want("pattern5")
    m = w["M"]
    lib = abi.load()
    G = eng.truss_graph(rp, ci, va)
    spare = 5
    names = ("truss", "support", "edge_u", "edge_v")
    vecs = {k: eng.alloc(m + spare) for k in names}
    short = eng.alloc(m - 1)
    mt, lv, rd, cp, tr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    scalars = (C.byref(mt), C.byref(lv), C.byref(rd), C.byref(cp), C.byref(tr))
    try:
        for mask in range(8):
            given = {"truss"} | {k for i, k in enumerate(names[1:]) if mask >> i & 1}
            for v in vecs.values():
                v.upload(np.full(m + spare, 7, np.int32))
            rc = lib.sh_truss(eng.h, G.h, *(vecs[k].h if k in given else None for k in names), m + 1, *scalars,
                              None, None, None, None, None)
            assert rc == abi.SH_OK
            assert (mt.value, lv.value, rd.value, cp.value, tr.value) == (w["max_truss"], w["levels"], w["rounds"], 1, w["triangles"])
            for k in names:
                d = vecs[k].download(np.int32)
                if k in given:
                    assert np.array_equal(d[:m], w[k]) and (d[m:] == 7).all(), k
                else:
                    assert (d == 7).all(), k
        short.upload(np.full(m - 1, 7, np.int32))
        for v in vecs.values():
            v.upload(np.full(m + spare, 7, np.int32))
        for bad in range(4):
            args = [short if i == bad else vecs[k] for i, k in enumerate(names)]
            with pytest.raises(EngineError) as err:
                eng.truss_numbers(G, *args)
            assert err.value.code == abi.SH_ESHAPE
        with pytest.raises(EngineError) as err:
            eng.truss_numbers(G, *(vecs[k] for k in names), max_rounds=-1)
        assert err.value.code == abi.SH_EINVAL
        for v in tuple(vecs.values()) + (short,):
            assert (v.download(np.int32) == 7).all()             # the buffers are untouched
    finally:
        for v in tuple(vecs.values()) + (short,):
            v.free()
        G.free()
