"""sh_tri on the GPU: tri, deg, the total and the number of edges against tests/tri_ref.py (pinned by
tests/test_tri_ref.py), against closed forms and against the host gold, under order = 0 and 1.

Every comparison of counts is exact (==): they are integers, and integer addition is associative whatever the lanes
race on.  The shapes are the smallest at which the kernels can still go wrong: forward lists on both sides of the
classes' limits (one lane up to 8 entries, one wave up to 512, a workgroup beyond, chunks of 2048), more rows than one
launch has lanes only where a case needs them (the friendship graphs, R-MAT-15).  K_2400 is the one large case: the only
way to a forward list beyond a chunk under order = 1, and a total above 2^31.
"""
from math import comb, isqrt

import numpy as np
import pytest

import tri_ref as T
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

ORDERS = (0, 1)
_cache, _want = {}, {}


def _loops():
    n = 1000
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)


MAKERS = {
    "no-rows": lambda: (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "empty": lambda: (5, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
    "loops": _loops,
    "pattern": T.pattern,
    "noise": lambda: T.with_noise(*T.pattern()),
    "one-way": T.one_way_triangles,
    "upper": lambda: T.upper_only(*T.pattern()),
    "lower": lambda: T.lower_only(*T.pattern()),
    "K9": lambda: T.complete(9),
    "K65": lambda: T.complete(65),
    "K300": lambda: T.complete(300),
    "limits": T.class_limits,
    "bipartite": lambda: T.bipartite(300, 300),
    "grid": lambda: T.triangulated_grid(128),
    "rmat12": lambda: (1 << 12,) + H.rmat(12, seed=40),
    "rmat15": lambda: (1 << 15,) + H.rmat(15, seed=40),
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
    """(tri, deg, M) of the reference, computed once per pattern and left unchanged."""
    if name not in _want:
        tri, deg, m = T.counts(*matrix(name))
        tri.setflags(write=False)
        deg.setflags(write=False)
        _want[name] = (tri, deg, m)
    return _want[name]


def symmetric(n, rp, ci, va):
    return T.from_pairs(n, *T.pairs_of(n, rp, ci, va))


def run(eng, mat, order, per_vertex=True, with_deg=True):
    """-> (tri, deg, triangles, probes, G.edges, G.max_forward) of one handle and one call."""
    n, rp, ci, va = mat
    G = eng.tri_graph(rp, ci, va, order=order)
    tv = eng.alloc(2 * n) if per_vertex else None
    dv = eng.alloc(n) if with_deg else None
    try:
        total, probes, _ = eng.triangles(G, tv, dv)
        tri = tv.download(np.uint32, 2 * n).view(np.uint64) if per_vertex else None
        deg = dv.download(np.int32, n) if with_deg else None
        return tri, deg, total, probes, G.edges, G.max_forward
    finally:
        for v in (tv, dv):
            if v is not None:
                v.free()
        G.free()


def check(eng, name, order, mat=None, w=None):
    wt, wd, wm = want(name) if w is None else w
    tri, deg, total, probes, edges, longest = run(eng, matrix(name) if mat is None else mat, order)
    assert np.array_equal(tri, wt) and np.array_equal(deg, wd)
    assert edges == wm and 3 * total == int(wt.sum())
    if order == 1:
        assert longest <= isqrt(2 * wm)
    return total, probes, longest


# ---- 1. trivial inputs
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["no-rows", "empty", "loops"])
def test_nothing_to_count(eng, name, order):
    total, probes, longest = check(eng, name, order)
    assert (total, probes, longest) == (0, 0, 0)


@pytest.mark.parametrize("order", ORDERS)
def test_noise_changes_nothing(eng, order):
    n, rp, ci, va = matrix("noise")
    assert T.counts(*T.noise_as_edges(n, rp, ci, va))[2] > want("pattern")[2]   # (it would change the graph if it counted)
    assert np.array_equal(want("noise")[0], want("pattern")[0])
    check(eng, "noise", order)
    check(eng, "pattern", order, mat=matrix("noise"))


# ---- 2. storage forms
@pytest.mark.parametrize("order", ORDERS)
def test_storage_forms_give_one_answer(eng, order):
    for form in ("pattern", "upper", "lower"):
        check(eng, "pattern", order, mat=matrix(form))
    total, _, _ = check(eng, "one-way", order)
    assert total >= 400
    check(eng, "one-way", order, mat=symmetric(*matrix("one-way")))


# ---- 3. complete graphs
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", [9, 65, 300])
def test_complete_graphs(eng, n, order):
    tri, deg, total, probes, edges, longest = run(eng, matrix(f"K{n}"), order)
    assert (tri == comb(n - 1, 2)).all() and (deg == n - 1).all()
    assert total == comb(n, 3) and int(tri.sum()) == 3 * total
    assert edges == comb(n, 2) and longest == n - 1
    check(eng, f"K{n}", order)


@pytest.mark.parametrize("order", ORDERS)
def test_k2400_total_above_2_to_31(eng, order):
    """K_2400: 2 879 400 edges, C(2400, 3) = 2 301 120 800 triangles (a signed 32-bit total would wrap), forward lists
    of every length up to 2399: both sides of every class limit and of the first chunk boundary, under either order.
    With tri under both orders.  The time of the call on an MI355X is unmeasured."""
    n = 2400
    if "K2400" not in _cache:
        _cache["K2400"] = T.complete(n)
    tri, deg, total, probes, edges, longest = run(eng, _cache["K2400"], order)
    assert total == comb(n, 3) == 2_301_120_800
    assert (tri == comb(n - 1, 2)).all() and (deg == n - 1).all()
    assert longest == n - 1 and edges == comb(n, 2)


# ---- 4. degree order
@pytest.mark.parametrize("hub", ["first", "last"])
def test_friendship_and_the_degree_order(eng, hub):
    k = 35_000
    mat = T.friendship(k, hub)
    n = mat[0]
    h = 0 if hub == "first" else n - 1
    got = {}
    for order in ORDERS:
        tri, deg, total, probes, edges, longest = run(eng, mat, order)
        assert total == k and tri[h] == k and deg[h] == 2 * k
        rest = np.delete(np.arange(n), h)
        assert (tri[rest] == 1).all() and (deg[rest] == 2).all() and edges == 3 * k
        got[order] = (probes, longest)
    assert got[1][1] <= isqrt(2 * 3 * k)
    if hub == "first":
        assert got[0][1] == 2 * k == 70_000
        assert got[1][0] < got[0][0]


# ---- 5. class limits
@pytest.mark.parametrize("order", ORDERS)
def test_class_limits(eng, order):
    total, probes, longest = check(eng, "limits", order)
    assert longest == (T.CHUNK + 1 if order == 0 else T.WAVE + 1)
    assert total == sum(L - 1 for L in T.CLASS_LENGTHS) + comb(T.SHORT + 2, 3) + comb(T.WAVE + 2, 3)


@pytest.mark.parametrize("order", ORDERS)
def test_bipartite_and_grid(eng, order):
    total, probes, _ = check(eng, "bipartite", order)
    assert total == 0 and probes > 0
    total, _, _ = check(eng, "grid", order)
    assert total == 2 * 127 ** 2


# ---- 6. R-MAT
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("scale", [12, 15])
def test_rmat(eng, scale, order):
    name = f"rmat{scale}"
    n, rp, ci, va = matrix(name)
    gold_tri, gold_deg = H.triangle_counts(rp, ci, va)
    wt, wd, _ = want(name)
    assert np.array_equal(gold_tri, wt) and np.array_equal(gold_deg, wd)
    total, _, _ = check(eng, name, order)                                  # as generated: one direction, duplicates
    assert total > 0
    assert check(eng, name, order, mat=symmetric(n, rp, ci, va))[0] == total


# ---- 7. the call's face
def test_optional_outputs_and_reuse(eng):
    n, rp, ci, va = matrix("rmat12")
    wt, wd, wm = want("rmat12")
    G = eng.tri_graph(rp, ci, va)                      # (order = 1 by default)
    spare = 5
    tv, dv = eng.alloc(2 * n + spare), eng.alloc(n + spare)
    try:
        tv.upload(np.full(2 * n + spare, 7, np.int32))
        dv.upload(np.full(n + spare, 7, np.int32))
        total, probes, _ = eng.triangles(G, tv, dv)
        t = tv.download(np.int32)
        d = dv.download(np.int32)
        assert np.array_equal(t[:2 * n].view(np.uint64), wt) and (t[2 * n:] == 7).all()
        assert np.array_equal(d[:n], wd) and (d[n:] == 7).all()
        assert 3 * total == int(wt.sum())
        assert eng.triangles(G)[:2][0] == total                      # tri = None, deg = None: the total alone
        assert eng.triangles(G, tv, None)[0] == total
        assert eng.triangles(G, None, dv)[0] == total
        for _ in range(3):                                           # a handle serves repeated calls
            assert eng.triangles(G, tv, dv)[:2] == (total, probes)
            assert np.array_equal(tv.download(np.int32)[:2 * n].view(np.uint64), wt)
        short_t, short_d = eng.alloc(2 * n - 1), eng.alloc(n - 1)
        try:
            short_t.upload(np.full(2 * n - 1, 7, np.int32))
            short_d.upload(np.full(n - 1, 7, np.int32))
            tv.upload(np.full(2 * n + spare, 7, np.int32))
            dv.upload(np.full(n + spare, 7, np.int32))
            for bad_t, bad_d in ((short_t, dv), (tv, short_d)):
                with pytest.raises(EngineError) as err:
                    eng.triangles(G, bad_t, bad_d)
                assert err.value.code == abi.SH_ESHAPE
            for v in (short_t, short_d, tv, dv):
                assert (v.download(np.int32) == 7).all()             # the buffers are untouched
        finally:
            short_t.free()
            short_d.free()
    finally:
        tv.free()
        dv.free()
        G.free()
    with pytest.raises(EngineError) as err:
        eng.tri_graph(rp, ci, va, order=2)
    assert err.value.code == abi.SH_EINVAL


# ---- 8. the footprint
@pytest.mark.parametrize("name", ["empty", "K65", "limits", "rmat12"])
def test_footprint_is_the_headers_formula(eng, name):
    n, rp, ci, va = matrix(name)
    for order in ORDERS:
        G = eng.tri_graph(rp, ci, va, order=order)
        try:
            edges = G.edges
            assert edges == want(name)[2]
            assert G.footprint == 4 * (n + 1) + 4 * n + 4 * edges + 33024
        finally:
            G.free()
