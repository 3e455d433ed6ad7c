"""sh_color on the GPU: the colours, the number of colours, the rounds, the coloured count and the records of every
round against tests/color_ref.py (pinned by tests/test_color_ref.py), against closed forms and against the host gold,
under the three orders and a prio vector.

Every comparison is exact (==): the colour of a vertex depends only on the colours of the neighbours that precede it,
so a graph and an order have one answer, whatever the lanes race on.  The shapes are the smallest at which the kernels
can still go wrong: lists on both sides of the classes' limits (one lane up to 8 entries, one wave up to 2048, a
workgroup beyond), colours beyond the first window of a long list, one word hit by 299 decrements, one hub of 70 001
entries, more rounds than a batch holds (the path)."""
import ctypes as C

import numpy as np
import pytest

import color_ref as K
import core_ref as R
import tri_ref as T
import wcc_ref as W
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

# (order, seed, with prio)
ORDERINGS = [(0, 0, False), (1, 12345, False), (2, 7, False), (1, 3, True)]
LIMITS = (8, 9, 64, 65, 2048, 2049)
# the clique inside the list of L entries: K_7 for the lane class (L = 8), K_70 for the others -- where a list of L
# entries can hold 70 and a leaf; where it cannot (L = 9, 64, 65) the largest clique that leaves one leaf, K_(L - 1)
LIMIT_K = tuple(7 if L <= K.SHORT else min(70, L - 1) for L in LIMITS)
_cache, _want = {}, {}


def _loops():
    n = 1000
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)


def _zeros():
    n, rp, ci, va = T.pattern(n=200, m=900, seed=4)
    return n, rp, ci, np.zeros(len(ci), np.float32)


MAKERS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "one-row": lambda: (1, np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "loops": _loops,
    "zeros": _zeros,
    "path": lambda: W.path(1000),
    "star": lambda: R.star(3000),
    "K9": lambda: T.complete(9),
    "K10": lambda: T.complete(10),
    "K5+ear": K.ear,
    "wheel": K.wheel,
    "grid16": lambda: W.grid(16),
    "rmat10": lambda: (1 << 10,) + H.rmat(10, seed=40),
    "messy": K.messy,
    "K70": lambda: T.complete(70),
    "K300": lambda: T.complete(300),
    "hub": R.big_hub,
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
    "rmat15": lambda: (1 << 15,) + H.rmat(15, seed=40),
    "tgrid256": lambda: T.triangulated_grid(256),
}
TRIVIAL = ("one-row", "loops", "zeros")
CPU_PATTERNS = ("path", "star", "K9", "K10", "K5+ear", "wheel", "grid16", "rmat10", "messy")


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


def tied_prio(n):
    return (np.random.default_rng(11).integers(-2, 3, n)).astype(np.int32)


def want(name, order, seed, prio=None, tag=None, mat=None, max_rounds=None):
    """The reference's answer and records, computed once per (pattern, order) and left unchanged."""
    key = (name, order, seed, tag, max_rounds)
    if key not in _want:
        r = K.schedule(*(matrix(name) if mat is None else mat), order=order, seed=seed, prio=prio, max_rounds=max_rounds)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _want[key] = r
    return _want[key]


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_color_abi.py asserts that the header states it)."""
    return 4 * (n + 1) + 16 * n + 8 * edges + 17408


def run(eng, mat, order=2, seed=0, prio=None, window=0, max_rounds=None, G=None):
    """-> dict of one call's outputs (on a handle of its own unless G is given)."""
    n = mat[0]
    own = G is None
    if own:
        G = eng.color_graph(*mat[1:])
    cv = eng.alloc(max(n, 1))
    pv = None
    try:
        cv.upload(np.full(max(n, 1), 7, np.int32))
        if prio is not None:
            pv = eng.alloc(max(n, 1))
            pv.upload(np.ascontiguousarray(prio, np.int32))
        colors, rounds, complete, coloured, sizes, edges, ns, total = eng.greedy_colors(
            G, cv, pv, order=order, seed=seed, window=window, max_rounds=max_rounds)
        return dict(color=cv.download(np.int32, n) if n else np.zeros(0, np.int32), colors=colors, rounds=rounds,
                    complete=complete, coloured=coloured, size=sizes, edges=edges, M=G.edges, max_degree=G.max_degree,
                    footprint=G.footprint)
    finally:
        cv.free()
        if pv is not None:
            pv.free()
        if own:
            G.free()


def same(got, w, n):
    assert np.array_equal(got["color"], w["color"])
    assert got["colors"] == w["colors"] and got["rounds"] == w["rounds"] and got["coloured"] == w["coloured"]
    assert got["complete"] is w["complete"]
    assert np.array_equal(got["size"], w["size"]) and np.array_equal(got["edges"], w["edges"])
    assert got["M"] == w["M"] and got["max_degree"] == w["max_degree"]
    assert got["footprint"] == header_footprint(n, w["M"])


def check(eng, name, order, seed, with_prio=False, window=0):
    mat = matrix(name)
    prio = tied_prio(mat[0]) if with_prio else None
    w = want(name, order, seed, prio, tag="prio" if with_prio else None)
    got = run(eng, mat, order, seed, prio, window)
    same(got, w, mat[0])
    assert got["complete"] is True and got["coloured"] == mat[0] and int(got["size"].sum()) == mat[0]
    return got


# ---- 1. nothing to colour
def test_no_rows(eng):
    got = run(eng, matrix("no-rows"))
    assert (got["colors"], got["rounds"], got["complete"], got["coloured"], got["M"]) == (0, 0, True, 0, 0)
    assert got["footprint"] == header_footprint(0, 0)


@pytest.mark.parametrize("order,seed,with_prio", ORDERINGS)
@pytest.mark.parametrize("name", TRIVIAL)
def test_nothing_to_colour(eng, name, order, seed, with_prio):
    got = check(eng, name, order, seed, with_prio)
    assert (got["color"] == 0).all() and got["colors"] == 1 and got["rounds"] == 1 and got["M"] == 0


# ---- 2. the patterns of the CPU tests
@pytest.mark.parametrize("order,seed,with_prio", ORDERINGS)
@pytest.mark.parametrize("name", CPU_PATTERNS + ("rmat12",))
def test_patterns(eng, name, order, seed, with_prio):
    check(eng, name, order, seed, with_prio)


# ---- 3. class limits: the last vertex in the order has a list of exactly L entries that hold a K_k
def test_class_limits(eng):
    n, rp, ci, va, hubs, prio = K.fans(LIMITS, LIMIT_K)
    mat = (n, rp, ci, np.ascontiguousarray(va))
    w = want("fans", 0, 0, prio, mat=mat)
    assert tuple(w["deg"][hubs].tolist()) == LIMITS and tuple(w["color"][hubs].tolist()) == LIMIT_K
    assert tuple(w["wait"][hubs].tolist()) == LIMITS          # every entry precedes the hub
    for order, seed in ((0, 0), (1, 5)):
        wo = want("fans", order, seed, prio, mat=mat)
        got = run(eng, mat, order, seed, prio)
        same(got, wo, n)
        assert tuple(got["color"][hubs].tolist()) == LIMIT_K


# ---- 4. cliques: n colours, n rounds, one word hit by up to n - 1 decrements
@pytest.mark.parametrize("name", ["K70", "K300"])
def test_cliques_and_the_decrement_race(eng, name):
    n = matrix(name)[0]
    first = check(eng, name, 1, 9)
    second = check(eng, name, 1, 9)
    assert first["colors"] == n and first["rounds"] == n and sorted(first["color"].tolist()) == list(range(n))
    for f in ("color", "size", "edges"):
        assert np.array_equal(first[f], second[f])


# ---- 5. windows: the colour of a long list lies beyond the first window
def test_windows(eng):
    n, rp, ci, va, hub, prio = K.fan(2130, 130)
    mat = (n, rp, ci, np.ascontiguousarray(va))
    w = want("fan2130", 0, 0, prio, mat=mat)
    assert w["color"][hub] == 130 and w["deg"][hub] == 2130
    for window in (64, 128, 0):
        got = run(eng, mat, 0, 0, prio, window=window)
        same(got, w, n)
        assert got["color"][hub] == 130


# ---- 6. more rounds than a batch holds
def test_path_in_natural_order_crosses_the_batch_seams(eng):
    got = check(eng, "path", 0, 0)
    assert got["rounds"] == 1000 and got["colors"] == 2 and (got["size"] == 1).all()
    assert got["color"].tolist() == [0, 1] * 500


# ---- 7. one long list
@pytest.mark.parametrize("order", [0, 2])
def test_hub_of_70001_leaves(eng, order):
    got = check(eng, "hub", order, 0)
    assert got["max_degree"] == 70_001 and got["rounds"] == 2 and got["colors"] == 2
    assert got["color"][0] == 0 and (got["color"][1:] == 1).all()


def test_hub_of_70001_leaves_coloured_last(eng):
    """The hub waits for all its leaves (its count comes from 35 pieces) and its one walk marks colour 0 70 001 times."""
    mat = matrix("hub")
    prio = np.zeros(mat[0], np.int32)
    prio[0] = -1
    w = want("hub", 0, 0, prio, tag="last")
    assert w["wait"][0] == 70_001 and w["color"][0] == 1
    same(run(eng, mat, 0, 0, prio), w, mat[0])


# ---- 8. max_rounds cuts a run short; the handle serves the next call
def test_cut_short_and_reuse(eng):
    mat = matrix("path")
    n = mat[0]
    full = want("path", 0, 0)
    part = want("path", 0, 0, max_rounds=3)
    G = eng.color_graph(*mat[1:])
    try:
        got = run(eng, mat, 0, 0, max_rounds=3, G=G)
        same(got, part, n)
        assert got["complete"] is False and got["coloured"] == 3 and got["rounds"] == 3
        assert got["color"][:3].tolist() == [0, 1, 0] and (got["color"][3:] == -1).all()
        again = run(eng, mat, 0, 0, G=G)
        same(again, full, n)
        other = run(eng, mat, 1, 4, G=G)
        same(other, want("path", 1, 4), n)
    finally:
        G.free()


# ---- 9. two handles, calls alternated
def test_two_handles_interleaved(eng):
    a, b = matrix("rmat12"), matrix("wheel")
    Ga, Gb = eng.color_graph(*a[1:]), eng.color_graph(*b[1:])
    try:
        for order, seed in ((2, 7), (0, 0), (2, 7)):
            ga = run(eng, a, order, seed, G=Ga)
            gb = run(eng, b, order, seed, G=Gb)
            same(ga, want("rmat12", order, seed), a[0])
            same(gb, want("wheel", order, seed), b[0])
    finally:
        Ga.free()
        Gb.free()


# ---- 10. the call's face
def test_optional_outputs_through_the_abi(eng):
    """coloured, prio and every per-round array NULL; vectors longer than rows keep their tail; short ones and bad
    scalars are refused with the buffers untouched."""
    n, rp, ci, va = matrix("rmat12")
    w = want("rmat12", 2, 7)
    prio = tied_prio(n)
    wp = want("rmat12", 1, 3, prio, tag="prio")
    lib = abi.load()
    G = eng.color_graph(rp, ci, va)
    spare = 5
    cv, pv, short = eng.alloc(n + spare), eng.alloc(n + spare), eng.alloc(n - 1)
    try:
        cv.upload(np.full(n + spare, 7, np.int32))
        k, rd, cp = C.c_int32(), C.c_int32(), C.c_int32()
        rc = lib.sh_color(eng.h, G.h, cv.h, None, 2, 7, 0, n + 1, C.byref(k), C.byref(rd), C.byref(cp),
                          None, None, None, None, None)
        assert rc == abi.SH_OK
        assert (k.value, rd.value, cp.value) == (w["colors"], w["rounds"], 1)
        c = cv.download(np.int32)
        assert np.array_equal(c[:n], w["color"]) and (c[n:] == 7).all()
        pv.upload(np.concatenate([prio, np.full(spare, 9, np.int32)]))
        eng.greedy_colors(G, cv, pv, order=1, seed=3)
        c, p = cv.download(np.int32), pv.download(np.int32)
        assert np.array_equal(c[:n], wp["color"]) and (c[n:] == 7).all()
        assert np.array_equal(p[:n], prio) and (p[n:] == 9).all()       # prio is only read
        short.upload(np.full(n - 1, 7, np.int32))
        cv.upload(np.full(n + spare, 7, np.int32))
        for bad_c, bad_p in ((short, pv), (cv, short)):
            with pytest.raises(EngineError) as err:
                eng.greedy_colors(G, bad_c, bad_p)
            assert err.value.code == abi.SH_ESHAPE
        for bad in (dict(order=3), dict(order=-1), dict(window=32), dict(window=96), dict(window=65536), dict(max_rounds=0)):
            with pytest.raises(EngineError) as err:
                eng.greedy_colors(G, cv, pv, **bad)
            assert err.value.code == abi.SH_EINVAL
        for v in (short, cv):
            assert (v.download(np.int32) == 7).all()                    # the buffers are untouched
    finally:
        for v in (cv, pv, short):
            v.free()
        G.free()


# ---- 11. against the host gold
@pytest.mark.parametrize("name", ["rmat15", "tgrid256"])
def test_against_the_host_gold(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.color_graph(rp, ci, va)
    try:
        for order, seed in ((0, 0), (1, 77), (2, 77)):
            color, colors, depth = H.greedy_colors(rp, ci, va, order=order, seed=seed)
            got = run(eng, matrix(name), order, seed, G=G)
            assert np.array_equal(got["color"], color) and got["colors"] == colors and got["complete"] is True
            assert got["rounds"] == int(depth.max()) + 1 and got["coloured"] == n
            assert np.array_equal(got["size"], np.bincount(depth, minlength=got["rounds"]))
            assert got["colors"] <= got["max_degree"] + 1
    finally:
        G.free()
