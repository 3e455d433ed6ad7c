"""sh_bfs_levels on the GPU: levels, canonical parents, depth / reached / complete and the per-level bookkeeping, bit for
bit against a numpy BFS written from the definition in include/sparseharness_hip.h (itself cross-checked against
scipy.sparse.csgraph), under top-down only, bottom-up only, the default shares and one pair per matrix that changes
direction at least twice; against sh_iterate(SH_OR_AND_I32) and sh_bits_iterate on the same matrices; sources of every
kind, the level cap, reuse of a handle, a graph without rows, the footprint formula.

Every comparison is exact (== on int32 arrays): levels are unique, parents canonical.

A run can change direction twice only if it has three steps.  matrix4 (one step: vertex 0 reaches nobody) and matrix5
(two steps) cannot; for them the explicit pair is the one with the most changes there are (none / one), and the
assertion on two changes applies to every other matrix.
"""
import numpy as np
import pytest

import graph_patterns as P
from bfs_ref import DOWN_DEFAULT, UP_DEFAULT, Bfs, edges_of, oracle_bfs, predict_modes   # noqa: F401 (other test modules reach them here)
from conftest import MATRICES, mtx
from oracle import oracle as O
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

TOP_DOWN, BOTTOM_UP, DEFAULT = (1.0, 0.0), (0.0, 0.0), (-1.0, -1.0)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


rows_of_entries = P.rows_of_entries


def ragged_square():
    """P.ragged_pattern with small integer values, a third of them 0."""
    rng, rp, ci = P.ragged_pattern()
    va = rng.integers(0, 3, rp[-1]).astype(np.int32)   # a third of the stored values are 0
    return rp, ci, va


def grid_graph(h=200, w=300, seed=5):
    """4-neighbour grid, vertex (i, j) = i * w + j, integer weights 1..16."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src, dst = [], []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        src += [a.ravel(), b.ravel()]
        dst += [b.ravel(), a.ravel()]
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=h * w))]).astype(np.int32)
    va = np.random.default_rng(seed).integers(1, 17, len(dst)).astype(np.int32)
    return rp, dst.astype(np.int32), va


NAMES = MATRICES + ["ragged", "grid", "rmat17"]
_cache = {}


def matrix(name):
    """(n, row_ptr, col_idx, int32 values) of a test matrix."""
    if name not in _cache:
        if name == "ragged":
            rp, ci, va = ragged_square()
        elif name == "grid":
            rp, ci, va = grid_graph()
        elif name == "rmat17":   # long rows and long out-lists in both kernels
            rp, ci, va = H.rmat(17, seed=40)
            va = va.astype(np.int32)
        elif name == "edges":    # list lengths on the kernels' thresholds, all values 1
            rp, ci = P.edges_pattern()
            va = np.ones(len(ci), np.int32)
        else:
            rows, cols, _, rp, ci, va = H.mm_load(mtx(name), elem_is_int=True)
            assert rows == cols
        _cache[name] = (len(rp) - 1, rp, ci, np.ascontiguousarray(va, np.int32))
    return _cache[name]


# ------------------------------------------------------------------ the oracle: a BFS written from the definition (tests/bfs_ref.py)
def changes(modes):
    return int(np.count_nonzero(np.diff(modes))) if len(modes) > 1 else 0


def pair_with_two_changes(b):
    """(up_share, down_share) chosen from the oracle's own m_L / E and |F_L| / n: thresholds half-way between values
    that occur, and the pair under which the rule changes direction most often (the first of those)."""
    def mids(vals):
        v = np.unique(np.asarray(vals, np.float64))
        mid = (v[:-1] + v[1:]) / 2
        if len(mid) > 16:
            mid = mid[np.linspace(0, len(mid) - 1, 16).astype(int)]
        return list(mid)
    ups = mids(np.array(b.m) / max(b.E, 1)) or [0.5]
    downs = mids(np.array(b.sizes) / max(b.n, 1)) + [2.0]
    best = max(((changes(predict_modes(b, u, d)), -i, -j, u, d) for i, u in enumerate(ups) for j, d in enumerate(downs)))
    return best[3], best[4], best[0]


def test_the_oracle_agrees_with_scipy():
    """So that the oracle is not only our own reading of the definition (runs without a device, but lives here with
    the tests that rely on it)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    for name in MATRICES:
        n, rp, ci, va = matrix(name)
        c, r = edges_of(n, rp, ci, va)
        g = csr_matrix((np.ones(len(c)), (c, r)), shape=(n, n))   # entry (c, r): an edge from c to r
        dist, pred = shortest_path(g, method="D", directed=True, unweighted=True, indices=0, return_predecessors=True)
        b = oracle_bfs(n, rp, ci, va, O.initial_vector(O.OR_AND_I32, n))
        want = np.where(np.isinf(dist), -1, dist).astype(np.int32)
        np.testing.assert_array_equal(b.level, want)
        # scipy's predecessor is SOME parent: one level up and joined by an edge
        has = pred >= 0
        assert (has == (b.level > 0)).all()
        assert (b.level[pred[has]] == b.level[has] - 1).all()
    n, rp, ci, va = matrix("matrix2")
    b = oracle_bfs(n, rp, ci, va, O.initial_vector(O.OR_AND_I32, n))
    assert b.sizes[:-1] == [1, 43, 99, 1833, 9064, 5679, 989, 153, 37, 5] and b.depth == 9
    n, rp, ci, va = matrix("matrix")
    b = oracle_bfs(n, rp, ci, va, O.initial_vector(O.OR_AND_I32, n))
    assert (b.depth, b.reached, n) == (24, 1132, 1138)
    n, rp, ci, va = matrix("matrix5")
    assert oracle_bfs(n, rp, ci, va, O.initial_vector(O.OR_AND_I32, n)).reached == 4 and int((va == 0).sum()) == 1044


# ------------------------------------------------------------------ running it
def run(eng, G, x0, shares=DEFAULT, with_parent=True, cap=1 << 16):
    n = len(x0)
    xv, lv = eng.vector(np.asarray(x0, np.int32)), eng.alloc(max(n, 1)).fill(7, np.int32)
    pv = eng.alloc(max(n, 1)).fill(7, np.int32) if with_parent else None
    res = eng.bfs_levels(G, xv, lv, pv, max_levels=cap, up_share=shares[0], down_share=shares[1])
    level = lv.download(np.int32, n=n)
    parent = pv.download(np.int32, n=n) if with_parent else None
    np.testing.assert_array_equal(xv.download(np.int32, n=n), np.asarray(x0, np.int32))   # x0 is only read
    for v in (xv, lv, pv):
        if v is not None:
            v.free()
    return level, parent, res


def check(b, level, parent, res, shares, what=""):
    depth, reached, complete, modes, sizes, edges, per, total = res
    print(f"{what} shares {shares}: depth {depth} reached {reached} complete {complete} modes {list(modes[:12])} "
          f"sizes {list(sizes[:12])} edges {list(edges[:12])} total_ns {total}")
    np.testing.assert_array_equal(level, b.level, err_msg=f"{what} level, shares {shares}")
    if parent is not None:
        np.testing.assert_array_equal(parent, b.parent, err_msg=f"{what} parent, shares {shares}")
    assert (depth, reached, complete) == (b.depth, b.reached, b.complete), (what, shares)
    assert list(sizes) == b.sizes, (what, shares)
    assert len(modes) == len(edges) == len(per) == b.steps
    want_modes = predict_modes(b, *shares)
    assert list(modes) == want_modes, (what, shares)
    for L in range(b.steps):
        if modes[L] == 0:
            assert edges[L] == b.m[L], (what, shares, L)
        else:
            assert b.sizes[L + 1] <= edges[L] <= b.open_entries[L], (what, shares, L)
    assert total >= int(np.sum(per))


def source_vector(n, sources):
    x0 = np.zeros(n, np.int32)
    x0[list(sources)] = 1
    return x0


# ------------------------------------------------------------------ 1. every matrix, every way of choosing directions
@pytest.mark.parametrize("name", NAMES + ["edges"])
def test_levels_and_parents_in_every_direction(eng, name):
    n, rp, ci, va = matrix(name)
    if name == "edges":
        P.assert_edge_lengths(rp, ci)
    G = eng.bfs_graph(rp, ci, va)
    for source in P.sources(name):
        levels_and_parents_in_every_direction(eng, name, G, source)
    G.free()


def levels_and_parents_in_every_direction(eng, name, G, source):
    n, rp, ci, va = matrix(name)
    x0 = source_vector(n, [source])
    b = oracle_bfs(n, rp, ci, va, x0)
    assert G.edges == b.E
    up, down, n_changes = pair_with_two_changes(b)
    if b.steps >= 3:
        assert n_changes >= 2, f"{name}: no pair of shares changes direction twice ({b.m}, {b.sizes})"
    assert changes(predict_modes(b, *TOP_DOWN)) == 0 and not any(predict_modes(b, *TOP_DOWN))
    if b.m[0] > 0:   # (a source set without out-edges has m_0 = 0, which is not above 0 * E: its only step runs top-down)
        assert all(predict_modes(b, *BOTTOM_UP))
    for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT, (up, down)):
        level, parent, res = run(eng, G, x0, shares)
        check(b, level, parent, res, shares, name)
    level, parent, res = run(eng, G, x0, DEFAULT, with_parent=False)   # without the parent pass
    check(b, level, None, res, DEFAULT, name)
    if name == "ragged":
        assert b.indeg.max() > 4096 and b.outdeg.max() > 2048   # pieces in both kernels
    if name == "grid":
        assert b.depth == 498
    if name == "rmat17":
        assert b.indeg.max() > 32 and b.outdeg.max() > 2048


# ------------------------------------------------------------------ 2. against the entry points that exist
@pytest.mark.parametrize("name", NAMES)
def test_agrees_with_iterate_and_bits_iterate(eng, name):
    n, rp, ci, va = matrix(name)
    x0 = source_vector(n, [0])
    G = eng.bfs_graph(rp, ci, va)
    level, _, (depth, reached, complete, modes, sizes, edges, per, total) = run(eng, G, x0, DEFAULT, with_parent=False)
    assert complete
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
    iters, conv, _, _ = eng.iterate(O.OR_AND_I32, A, xv, yv, sc, 1, 1, max_iters=5000)
    x = xv.download(np.int32)
    assert conv and iters == depth + 1
    np.testing.assert_array_equal(level >= 0, x != 0)
    for v in (xv, yv, sc):
        v.free()
    # bit 0 of the one word per vertex carries the source; the other 31 sources are empty
    P0 = x0.astype(np.uint32)
    xv, yv, sc = eng.vector(P0), eng.vector(P0), eng.alloc(n).fill(0)
    launches, b_iters, b_conv, _, _, newly = eng.bits_iterate(A, xv, yv, sc, 1, 1, 1, max_iters=5000, counts=True)
    assert b_iters[0] == depth + 1 and b_conv[0]
    assert list(sizes[1:]) == [int(k) for k in newly[:depth + 1, 0]]
    for v in (xv, yv, sc):
        v.free()
    A.free()
    G.free()


# ------------------------------------------------------------------ 3. sources of every kind
@pytest.mark.parametrize("name", ["matrix", "matrix2", "ragged", "grid", "rmat17"])
def test_sources(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.bfs_graph(rp, ci, va)
    c, _ = edges_of(n, rp, ci, va)
    outdeg = np.bincount(c, minlength=n)
    rng = np.random.default_rng(11)
    cases = {"seven": rng.choice(n, 7, replace=False), "all": np.arange(n), "none": []}
    if name in ("matrix", "rmat17"):   # (the other three have no vertex with an empty out-list)
        cases["leaf"] = [int(np.flatnonzero(outdeg == 0)[0])]
    for what, sources in cases.items():
        x0 = source_vector(n, sources)
        b = oracle_bfs(n, rp, ci, va, x0)
        for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
            level, parent, res = run(eng, G, x0, shares)
            check(b, level, parent, res, shares, f"{name} {what}")
        if what == "all":
            assert b.depth == 0 and b.reached == n and b.steps == 1 and b.complete
        if what == "none":
            assert b.reached == 0 and b.steps == 0 and b.complete and (b.level == -1).all()
        if what == "leaf":
            assert b.reached == 1 and b.steps == 1
    # x0 values other than 1 are sources too
    x0 = np.zeros(n, np.int32)
    x0[[3, 5]] = [-7, 1 << 30]
    b = oracle_bfs(n, rp, ci, va, x0)
    level, parent, res = run(eng, G, x0)
    check(b, level, parent, res, DEFAULT, f"{name} odd source values")
    G.free()


# ------------------------------------------------------------------ 4. the level cap
@pytest.mark.parametrize("name", ["matrix", "matrix2", "grid", "rmat17"])
def test_cap(eng, name):
    n, rp, ci, va = matrix(name)
    x0 = source_vector(n, [0])
    full = oracle_bfs(n, rp, ci, va, x0)
    G = eng.bfs_graph(rp, ci, va)
    for cap in sorted({1, 2, full.depth // 2, full.depth - 1, full.depth, full.depth + 1, full.depth + 40}):
        if cap < 1:
            continue
        b = oracle_bfs(n, rp, ci, va, x0, max_levels=cap)
        assert b.complete == (cap > full.depth)   # cut at the depth: every level assigned, the empty frontier not seen
        np.testing.assert_array_equal(b.level, np.where(full.level <= cap, full.level, -1))
        for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
            level, parent, res = run(eng, G, x0, shares, cap=cap)
            check(b, level, parent, res, shares, f"{name} cap {cap}")
    G.free()


# ------------------------------------------------------------------ 5. reuse, no rows, footprint, errors
def test_a_handle_serves_many_calls(eng):
    n, rp, ci, va = matrix("grid")
    G = eng.bfs_graph(rp, ci, va)
    for source in (0, n - 1, n // 2 + 17, 0):
        x0 = source_vector(n, [source])
        b = oracle_bfs(n, rp, ci, va, x0)
        fresh = eng.bfs_graph(rp, ci, va)
        for handle in (G, fresh):
            for shares in (DEFAULT, BOTTOM_UP, pair_with_two_changes(b)[:2]):
                level, parent, res = run(eng, handle, x0, shares)
                check(b, level, parent, res, shares, f"grid from {source}")
        fresh.free()
    # a capped call leaves a frontier behind: the next call must not see it
    x0 = source_vector(n, [0])
    run(eng, G, x0, BOTTOM_UP, cap=5)
    run(eng, G, x0, TOP_DOWN, cap=6)
    b = oracle_bfs(n, rp, ci, va, source_vector(n, [n - 1]))
    for shares in (BOTTOM_UP, TOP_DOWN):
        level, parent, res = run(eng, G, source_vector(n, [n - 1]), shares)
        check(b, level, parent, res, shares, "grid after capped calls")
    G.free()


def test_a_graph_without_rows(eng):
    rp = np.zeros(1, np.int32)
    G = eng.bfs_graph(rp, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert G.edges == 0 and G.footprint == footprint_formula(0, 0)
    xv, lv = eng.alloc(1), eng.alloc(1)
    depth, reached, complete, modes, sizes, edges, per, total = eng.bfs_levels(G, xv, lv, None, max_levels=10)
    assert (depth, reached, complete, len(modes), total) == (0, 0, True, 0, 0)
    for h in (xv, lv, G):
        h.free()
    # rows without a single entry
    n = 100
    G = eng.bfs_graph(np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    x0 = source_vector(n, [3, 4])
    b = oracle_bfs(n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), x0)
    for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
        level, parent, res = run(eng, G, x0, shares)
        check(b, level, parent, res, shares, "no entries")
    G.free()


def footprint_formula(rows, edges):
    w = (rows + 31) // 32
    return 8 * (rows + 1) + 8 * edges + 8 * rows + 8 * w + 16 * (edges // 1024 + 1) + 8 * (edges // 2048 + 1) + 18432


@pytest.mark.parametrize("name", NAMES)
def test_footprint_is_the_documented_formula_and_edges_are_counted(eng, name):
    n, rp, ci, va = matrix(name)
    G = eng.bfs_graph(rp, ci, va)
    E = len(edges_of(n, rp, ci, va)[0])
    assert G.edges == E
    assert G.footprint == footprint_formula(n, E)
    if name == "matrix5":
        assert E < len(ci) - 1000   # the edge filter is really exercised
    G.free()


def test_float_values_and_minus_zero(eng):
    """The filter looks at the 32 value bits: -0.0f is non-zero as an int32 and is an edge, +0.0f is none."""
    n = 6
    rows = [[], [0], [1], [2], [3], [4]]   # a path 0 -> 1 -> ... -> 5
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate([np.array(r, np.int32) for r in rows]).astype(np.int32)
    va = np.array([1.5, -0.0, 2.0, 0.0, 1.0], np.float32)   # the edge 3 -> 4 is a stored zero
    x0 = source_vector(n, [0])
    b = oracle_bfs(n, rp, ci, va, x0)
    assert list(b.level) == [0, 1, 2, 3, -1, -1] and b.E == 4
    G = eng.bfs_graph(rp, ci, va)
    assert G.edges == 4
    for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
        level, parent, res = run(eng, G, x0, shares)
        check(b, level, parent, res, shares, "path")
    G.free()


def test_errors(eng):
    n, rp, ci, va = matrix("matrix3")
    G = eng.bfs_graph(rp, ci, va)
    xv, lv, pv, short = eng.alloc(n).fill(0), eng.alloc(n), eng.alloc(n), eng.alloc(n - 1)
    with pytest.raises(EngineError, match="alias"):
        eng.bfs_levels(G, xv, xv, None, max_levels=10)
    with pytest.raises(EngineError, match="alias"):
        eng.bfs_levels(G, xv, lv, lv, max_levels=10)
    with pytest.raises(EngineError, match="alias"):
        eng.bfs_levels(G, xv, lv, xv, max_levels=10)
    with pytest.raises(EngineError, match="level is shorter"):
        eng.bfs_levels(G, xv, short, None, max_levels=10)
    with pytest.raises(EngineError, match="parent is shorter"):
        eng.bfs_levels(G, xv, lv, short, max_levels=10)
    with pytest.raises(EngineError, match="x0 is shorter"):
        eng.bfs_levels(G, short, lv, None, max_levels=10)
    with pytest.raises(EngineError, match="max_levels"):
        eng.bfs_levels(G, xv, lv, pv, max_levels=0)
    with pytest.raises(EngineError, match="NaN"):
        eng.bfs_levels(G, xv, lv, pv, max_levels=10, up_share=float("nan"))
    bad = rp.copy()
    bad[-1] += 1
    with pytest.raises(EngineError, match="row_ptr"):
        eng.bfs_graph(bad, ci, va)
    for h in (G, xv, lv, pv, short):
        h.free()
