"""Every small graph at once: the enumeration, the disjoint union as one CSR matrix, and a reference of each graph entry
point written from the definitions in include/sparseharness_hip.h as numpy over (G, n, n) tensors.  Not a test, not a
conftest: tests/test_small_graphs_ref.py pins what is here against the project's other references and scipy,
tests/test_small_graphs_gpu.py compares the engine with it.  Nothing here calls scc_ref, wcc_ref, tri_ref, core_ref,
truss_ref, sssp_ref, color_ref, msf_ref, match_ref, rcm_ref or oracle_bfs, and no line is shared with the product.
sh_rcm alone has no tensor form here: its walk in (deg, index) order runs over the whole union, so its tests take
rcm_ref.serial and rcm_ref.levels on the union as one matrix.

Conventions.  A[g, r, c] is true when row r of graph g stores column c: in the header's words the edge c -> r.  A "local"
answer is a (G, n) array that speaks of the vertices 0 .. n - 1 of each graph on its own (a parent, a label: a local
index or -1); to_global() turns it into what the engine must return for the union under a numbering:

  "blocks":  vertex v of graph g is g * n + v -- the vertices of a graph sit in neighbouring lanes;
  "strided": vertex v of graph g is v * G + g -- the vertices of a graph sit in different workgroups, so the races of a
             round cross workgroups.

Both keep the local order inside a graph (u < v locally iff globally), so every "smallest" and "largest" rule of the
header gives the same local answer under either.  Not so the ties that hash an id: orders 1 and 2 of sh_color compare
mix32(v ^ seed) of the union's vertex index, sh_match with seed != 0 mix32(e ^ seed) of the union's edge id, so there
the order inside a graph differs between the two numberings, and the references take the union's ids.
"""
import numpy as np

FLT_MAX = np.float32(3.4028235e38)
NUMBERINGS = ("blocks", "strided")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ enumeration
def all_digraphs(n, loops=True):
    """(G, n, n) bool, G = 2^(n * n) (2^(n * (n - 1)) without loops): bit b of g selects the b-th (r, c) position in
    row-major order."""
    pos = [(r, c) for r in range(n) for c in range(n) if loops or r != c]
    g = np.arange(1 << len(pos), dtype=np.int64)
    A = np.zeros((len(g), n, n), bool)
    for b, (r, c) in enumerate(pos):
        A[:, r, c] = (g >> b) & 1
    return A


def all_undirected(n):
    """(G, n, n) bool, symmetric, G = 2^(n * (n - 1) / 2): bit b of g selects the b-th pair u < v."""
    pairs = [(u, v) for u in range(n) for v in range(u + 1, n)]
    g = np.arange(1 << len(pairs), dtype=np.int64)
    A = np.zeros((len(g), n, n), bool)
    for b, (u, v) in enumerate(pairs):
        A[:, u, v] = A[:, v, u] = (g >> b) & 1
    return A


def halves(A):
    """Which of a symmetric pair is written: graphs of even g store the upper triangle only (r < c), odd ones the lower."""
    G, n, _ = A.shape
    upper = np.triu(np.ones((n, n), bool), 1)
    even = (np.arange(G) % 2 == 0)[:, None, None]
    return np.where(even, upper[None], upper.T[None])


# ------------------------------------------------------------------ the union and its numberings
def vertex_ids(G, n, numbering):
    """(G, n) int64: the index of vertex v of graph g in the union."""
    g, v = np.arange(G, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    if numbering == "blocks":
        return g * n + v
    assert numbering == "strided"
    return v * G + g


def scatter(values, numbering):
    """A (G, n) array as the union's vector (element vertex_ids[g, v] = values[g, v])."""
    values = np.asarray(values)
    return np.ascontiguousarray(values if numbering == "blocks" else values.T).reshape(-1)


def gather(vector, G, n, numbering):
    """The union's vector as a (G, n) array: the inverse of scatter."""
    vector = np.asarray(vector)
    return vector.reshape(G, n) if numbering == "blocks" else vector.reshape(n, G).T


def to_global(local, numbering):
    """A (G, n) array of local vertex indices (-1: none) as the union's vector of union indices (-1 kept)."""
    local = np.asarray(local, np.int64)
    G, n = local.shape
    ids = vertex_ids(G, n, numbering)
    return scatter(np.where(local >= 0, np.take_along_axis(ids, np.maximum(local, 0), axis=1), -1), numbering)


def union(A, numbering, stored=None):
    """-> (row_ptr, col_idx, (g, r, c)): the disjoint union of the graphs of A as one CSR pattern (int32) and the local
    position of every entry.  stored (a (G, n, n) mask) selects which of the entries of A are written.  The entries of a
    row keep their local order (ascending c)."""
    G, n, _ = A.shape
    g, r, c = np.nonzero(A if stored is None else A & stored)
    ids = vertex_ids(G, n, numbering)
    row, col = ids[g, r], ids[g, c]
    order = np.argsort(row, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=G * n))])
    assert rp[-1] == len(col) < 2 ** 31
    return rp.astype(np.int32), col[order].astype(np.int32), (g[order], r[order], c[order])


# ------------------------------------------------------------------ reachability: scc and wcc
def closure(A):
    """R[g, r, c]: c reaches r in graph g, every vertex reaching itself (Warshall)."""
    G, n, _ = A.shape
    R = A | np.eye(n, dtype=bool)[None]
    for k in range(n):
        R = R | (R[:, :, k:k + 1] & R[:, k:k + 1, :])
    return R


def _largest_mutual(R):
    n = R.shape[1]
    mutual = R & R.transpose(0, 2, 1)
    return np.where(mutual, np.arange(n)[None, None, :], -1).max(axis=2)


def scc(A):
    """(G, n) local: the largest u such that v reaches u and u reaches v."""
    return _largest_mutual(closure(A))


def wcc(A):
    """(G, n) local: the same on the symmetrised pattern."""
    return _largest_mutual(closure(A | A.transpose(0, 2, 1)))


# ------------------------------------------------------------------ BFS
def sources(G, n):
    """(first, second) masks (G, n): every graph has one source on vertex g % n; every third graph a second one on
    another vertex."""
    g = np.arange(G)
    first = np.zeros((G, n), bool)
    first[g, g % n] = True
    second = np.zeros((G, n), bool)
    third = g[g % 3 == 0]
    second[third, (third % n + 1 + (third // 3) % (n - 1)) % n] = True
    assert not (first & second).any()
    return first, second


def bfs(A, src):
    """Levels by n boolean steps out of the source mask, parents by the rule.  -> dict(level, parent, parent_largest
    (all (G, n), local), depth, reached, sizes, edges): sizes / edges as sh_bfs_levels reports size_per_level /
    edges_per_level of a complete top-down run over the union (one step per level, the last assigning nothing)."""
    G, n, _ = A.shape
    level = np.where(src, 0, -1)
    frontier = src.copy()
    for step in range(n):
        new = (A & frontier[:, None, :]).any(axis=2) & (level == -1)
        level[new] = step + 1
        frontier = new
    assert not frontier.any()
    up = A & (level[:, :, None] > 0) & (level[:, None, :] == level[:, :, None] - 1)   # [g, r, c]: c is one level up
    has = up.any(axis=2)
    assert (has == (level > 0)).all()
    parent = np.where(has, up.argmax(axis=2), -1)
    parent_largest = np.where(has, n - 1 - up[:, :, ::-1].argmax(axis=2), -1)
    depth = int(level.max())
    outdeg = A.sum(axis=1)   # [g, c]: the entries that store column c
    sizes = [int((level == k).sum()) for k in range(depth + 1)] + [0]
    edges = [int(outdeg[level == k].sum()) for k in range(depth + 1)]
    return dict(level=level, parent=parent, parent_largest=parent_largest, depth=depth, reached=int((level >= 0).sum()),
                sizes=sizes, edges=edges)


# ------------------------------------------------------------------ SSSP
T = np.float32(2.0 ** -30)   # below half an ulp of every distance >= 0.5
# weight of the entry at position (r, c), whatever the graph: zeros on a diagonal and an off-diagonal position, T on
# both kinds, and 0.5 / 1 / 2 / 3 so that many pairs of paths tie after rounding (1 + 2 = 3, 0.5 + 0.5 = 1, x + T = x)
TABLE = np.array([[T,   1,   0.5, 3,   1,   2],
                  [1,   0,   T,   0.5, 2,   0.5],
                  [0,   2,   1,   0.5, 3,   1],
                  [3,   2,   0.5, 0,   1,   T],
                  [0.5, 1,   2,   T,   0.5, 3],
                  [2,   3,   1,   1,   0,   1]], np.float32)
SMALLEST_WEIGHT = T
SECOND_START = np.float32(0.75)


def sssp_inputs(G, n):
    """-> (val, x0, src): val (G, n, n) float32, the value stored at every position -- TABLE, negated in every fifth
    graph (the header takes |a|; a negated zero is -0.0, still an edge of weight 0); x0 (G, n) float32: 0 on the first
    source, SECOND_START on the second (negated in odd graphs: the start is |x0|), FLT_MAX elsewhere; src = the sources."""
    assert n <= len(TABLE)
    sign = np.where(np.arange(G) % 5 == 0, np.float32(-1), np.float32(1))
    val = TABLE[None, :n, :n] * sign[:, None, None]
    first, second = sources(G, n)
    x0 = np.full((G, n), FLT_MAX, np.float32)
    x0[first] = 0
    x0[second] = SECOND_START
    x0[second & (np.arange(G) % 2 == 1)[:, None]] = -SECOND_START
    assert val.dtype == np.float32
    return val, x0, first | second


def sssp(A, val, x0):
    """F <- min(F, min_c fl32(F[c] + |val[r, c]|)) in float32 from d0 = |x0| until no bit changes; pred by the rule.
    -> dict(dist (G, n) float32, pred, pred_largest (local), d0, reached, sweeps, out_degrees_of_reached)."""
    G, n, _ = A.shape
    w = np.abs(np.asarray(val, np.float32))
    edge = A & np.isfinite(w)
    d0 = np.minimum(np.abs(np.asarray(x0, np.float32)), FLT_MAX)
    F, sweeps = d0.copy(), 0

    def through_of(F):
        with np.errstate(over="ignore"):
            t = F[:, None, :] + w   # [g, r, c] = fl32(F[g, c] + w[g, r, c]): one float32 addition, rounded once
        assert t.dtype == np.float32
        return t

    while True:
        t = np.where(edge, np.minimum(through_of(F), FLT_MAX), FLT_MAX)   # a sum that overflows stays FLT_MAX
        nxt = np.minimum(F, t.min(axis=2))
        if np.array_equal(bits(nxt), bits(F)):
            break
        F, sweeps = nxt, sweeps + 1
    moved = bits(F) != bits(d0)
    hit = edge & moved[:, :, None] & (bits(through_of(F)) == bits(F)[:, :, None])
    has = hit.any(axis=2)
    assert (has == moved).all(), "at a fixed point every moved vertex has a predecessor"
    pred = np.where(has, hit.argmax(axis=2), -1)
    pred_largest = np.where(has, n - 1 - hit[:, :, ::-1].argmax(axis=2), -1)
    reached = F < FLT_MAX
    outdeg = edge.sum(axis=1)
    return dict(dist=F, pred=pred, pred_largest=pred_largest, d0=d0, reached=int(reached.sum()), sweeps=sweeps,
                out_degrees_of_reached=int(outdeg[reached].sum()))


# ------------------------------------------------------------------ the simple undirected graph: triangles, core, truss
def simple(A):
    """The symmetrised, loop-free pattern."""
    n = A.shape[1]
    return (A | A.transpose(0, 2, 1)) & ~np.eye(n, dtype=bool)[None]


def triangles(A):
    """-> dict(tri (G, n) int64 = diag(S^3) / 2, deg (G, n), total)."""
    S = simple(A).astype(np.int64)
    walks = np.einsum("gij,gji->gi", S @ S, S)
    assert (walks % 2 == 0).all()
    tri = walks // 2
    assert int(tri.sum()) % 3 == 0
    return dict(tri=tri, deg=S.sum(axis=2), total=int(tri.sum()) // 3)


def core(A):
    """Peel k = 1 .. n - 1, each to its fixed point: core[v] = the last k whose peel v survived.  -> dict(core (G, n),
    degeneracy)."""
    S = simple(A)
    G, n, _ = S.shape
    alive, number = np.ones((G, n), bool), np.zeros((G, n), np.int64)
    for k in range(1, n):
        while True:
            drop = alive & ((S & alive[:, None, :]).sum(axis=2) < k)
            if not drop.any():
                break
            alive &= ~drop
        number[alive] = k
    return dict(core=number, degeneracy=int(number.max()))


def edges(A, numbering):
    """The union's edge list in the header's order: edge e is the e-th smallest pair u < v of union indices.  -> dict(
    edge_u, edge_v (int32, per edge), graph, lu, lv (the graph and the local ends lu < lv of every edge), M)."""
    S = simple(A)
    G, n, _ = S.shape
    g, u, v = np.nonzero(S & np.triu(np.ones((n, n), bool), 1)[None])
    ids = vertex_ids(G, n, numbering)
    gu, gv = ids[g, u], ids[g, v]
    order = np.lexsort((gv, gu))
    g, u, v, gu, gv = g[order], u[order], v[order], gu[order], gv[order]
    assert (gu < gv).all()
    return dict(edge_u=gu.astype(np.int32), edge_v=gv.astype(np.int32), graph=g, lu=u, lv=v, M=len(g))


def truss(A, numbering):
    """support = (S @ S) * S; peel k = 3 .. n + 1, each to its fixed point: truss[e] = the last k whose peel e survived,
    2 for an edge that survived none.  -> dict(truss, support, edge_u, edge_v (per edge of the union in the header's
    order: edge e is the e-th smallest pair u < v of union indices), graph, lu, lv (the graph and local ends of every
    edge), max_truss, triangles, M)."""
    S = simple(A)
    G, n, _ = S.shape
    Si = S.astype(np.int64)
    support = (Si @ Si) * Si
    E, number = S.copy(), np.where(S, 2, 0)
    for k in range(3, n + 2):
        while True:
            Ei = E.astype(np.int64)
            drop = E & ((Ei @ Ei) * Ei < k - 2)
            if not drop.any():
                break
            E &= ~drop
        number[E] = k
    assert not E.any()   # K_n has truss n: nothing survives the peel of n + 1
    e = edges(S, numbering)
    g, u, v, gu, gv = e["graph"], e["lu"], e["lv"], e["edge_u"], e["edge_v"]
    total = int(support.sum())
    assert total % 6 == 0   # every triangle is counted at its three edges, each seen from both ends
    return dict(truss=number[g, u, v].astype(np.int32), support=support[g, u, v].astype(np.int32),
                edge_u=gu, edge_v=gv, graph=g, lu=u, lv=v,
                max_truss=int(number.max()), triangles=total // 6, M=len(g))


# ------------------------------------------------------------------ greedy colouring in a fixed order
def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 words (uint64 in numpy)."""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x).astype(np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def color_keys(A, numbering, order, seed, prio=None, tie="header", ids="global"):
    """(G, n) int64: vertex v precedes u exactly when key[v] > key[u].  The primary is prio ((G, n)) when given, the
    degree for order 2, else 0; the tie is built from the UNION's index of the vertex: the smaller index first for order
    0, the larger mix32(v ^ seed) first for orders 1 and 2.  tie = "larger" (the larger index first, under order 0) and
    ids = "local" (the tie from the local index) are broken on purpose (tests/test_small_graphs_ref.py)."""
    assert order in (0, 1, 2)
    G, n, _ = A.shape
    v = vertex_ids(G, n, numbering) if ids == "global" else np.tile(np.arange(n, dtype=np.int64), (G, 1))
    primary = np.asarray(prio, np.int64) if prio is not None else (simple(A).sum(axis=2).astype(np.int64) if order == 2 else np.zeros((G, n), np.int64))
    if order == 0:
        low = v if tie == "larger" else (1 << 32) - 1 - v
    else:
        low = mix32(v ^ (int(seed) & 0xFFFFFFFF)).astype(np.int64)
    return primary * (1 << 32) + low


def prio_of(G, n):
    """(G, n) int32: a priority vector with ties inside a graph (so that the order below it still decides), a negative
    value, and another pattern from graph to graph."""
    g, v = np.arange(G, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    return ((v * 3 + g) % 4 - 1).astype(np.int32)


def coloring(A, key):
    """n steps per graph: the uncoloured vertex of the largest key takes the smallest colour that none of its coloured
    neighbours holds.  -> dict(color (G, n) local, colors, depth (G, n): the longest chain of preceding neighbours that
    ends in the vertex, counted from 0)."""
    S = simple(A)
    G, n, _ = S.shape
    key = np.asarray(key, np.int64)
    color, depth = np.full((G, n), -1, np.int64), np.zeros((G, n), np.int64)
    rows = np.arange(G)
    for _ in range(n):
        v = np.where(color < 0, key, np.iinfo(np.int64).min).argmax(axis=1)
        assert (color[rows, v] < 0).all()
        before = S[rows, v, :] & (color >= 0)                                 # (G, n): the coloured neighbours
        held = (before[:, :, None] & (color[:, :, None] == np.arange(n + 1)[None, None, :])).any(axis=1)
        color[rows, v] = held.argmin(axis=1)                                  # (n neighbours cannot hold n + 1 colours)
        depth[rows, v] = np.where(before.any(axis=1), np.where(before, depth, -1).max(axis=1) + 1, 0)
    return dict(color=color, colors=int(color.max()) + 1, depth=depth)


# ------------------------------------------------------------------ weights by bit pattern: forest and matching
_ONE, _TWO, _HALF, _THREE = 0x3F800000, 0x40000000, 0x3F000000, 0x40400000
_NEG, _MZERO, _PZERO, _INF, _NAN = 0xBFC00000, 0x80000000, 0x00000000, 0x7F800000, 0x7FC00001   # -1.5, -0.0, +0.0, +inf, a NaN
# the 32 bits stored at position (r, c) of the base table: most pairs asymmetric ((0, 1): 2 and 1), many pairs of equal
# weight (1 and 0.5 throughout), -1.5 at (0, 3) and (4, 2), -0.0 at (2, 3), +inf at (0, 4) and on both sides of (4, 5), a
# NaN at (1, 5), and ONE stored +0.0 at (1, 2): no entry by the graph rule, so {1, 2} is an edge only through (2, 1)
WBITS = np.array([[_ONE,  _TWO,   _ONE,   _NEG,   _INF,  _HALF],
                  [_ONE,  _THREE, _PZERO, _TWO,   _ONE,  _NAN],
                  [_TWO,  _HALF,  _ONE,   _MZERO, _TWO,  _ONE],
                  [_ONE,  _TWO,   _ONE,   _HALF,  _HALF, _TWO],
                  [_HALF, _ONE,   _NEG,   _TWO,   _ONE,  _INF],
                  [_TWO,  _ONE,   _ONE,   _HALF,  _INF,  _ONE]], np.uint32)


def order_key(b):
    """k(b) of the header on uint32 bits: b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000."""
    b = np.asarray(b, np.uint32)
    return np.where(b >> np.uint32(31) != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def weights(G, n):
    """(G, n, n) float32, the value stored at every position: graph g reads WBITS rotated by g % 6 along both axes (so
    that the 3 and 4 vertices of a small graph meet every special value in some graph), with the sign bit of every value
    flipped in every fifth graph (the order of the weights turns round; +0.0 becomes -0.0, which counts, and -0.0
    becomes the stored zero).  Only bits are moved: no arithmetic touches the NaN."""
    assert n <= len(WBITS)
    g = np.arange(G)[:, None, None]
    r, c = np.arange(n)[None, :, None], np.arange(n)[None, None, :]
    b = WBITS[(r + g) % 6, (c + g) % 6]
    b = np.where(g % 5 == 0, b ^ np.uint32(0x80000000), b).astype(np.uint32)
    return np.ascontiguousarray(b).view(np.float32)


def edge_weights(A, val, numbering, entry="smallest", zero_counts=False):
    """The weighted graph of sh_msf and sh_match: an entry counts when it is stored and its 32 bits are not all zero; the
    weight of a pair is the smallest counting entry of its two positions by k.  -> edges() of the counting pattern, with
    k (uint32 per edge) and weight (the 32 bits of the chosen entry).  entry = "first" (the entry met first in the
    row-major order of the matrix, that of the smaller row) and zero_counts are broken on purpose."""
    b = bits(val).reshape(np.asarray(val).shape)
    counts = A & ((b != 0) | zero_counts)
    e = edges(counts, numbering)
    g, u, v = e["graph"], e["lu"], e["lv"]
    top = np.uint64(1) << np.uint64(32)   # (above every k: a position that does not count)
    ku = np.where(counts[g, u, v], order_key(b[g, u, v]).astype(np.uint64), top)   # the entry in the smaller row
    kv = np.where(counts[g, v, u], order_key(b[g, v, u]).astype(np.uint64), top)
    use_u = (ku <= kv) if entry == "smallest" else counts[g, u, v]
    e["k"] = np.where(use_u, ku, kv).astype(np.uint32)
    e["weight"] = np.where(use_u, b[g, u, v], b[g, v, u]).astype(np.uint32)
    return e


def _ranks(graph, key):
    """The rank of every edge among the edges of its graph in ascending key, and the largest number of edges of a graph."""
    order = np.lexsort((key, graph))
    start = np.concatenate([[0], np.cumsum(np.bincount(graph))])[graph[order]] if len(graph) else np.zeros(0, np.int64)
    rank = np.empty(len(graph), np.int64)
    rank[order] = np.arange(len(graph)) - start
    return rank, (int(rank.max()) + 1 if len(graph) else 0)


def msf(A, val, numbering, tie="header", **broken):
    """Kruskal in every graph at once: the edges in ascending KEY(e) = k(weight[e]) << 32 | e, e the union's edge id; step
    j takes the j-th edge of every graph and keeps it when its ends carry different labels.  A label is the largest index
    of the component so far.  -> dict(in_msf (per edge), comp (G, n) local, tree_edges, components, k, weight and the
    fields of edges()).  tie = "larger" (KEY's low word ~e) and **broken (edge_weights) are wrong on purpose."""
    G, n, _ = A.shape
    e = edge_weights(A, val, numbering, **broken)
    ids = np.arange(e["M"], dtype=np.uint64)
    key = (e["k"].astype(np.uint64) << np.uint64(32)) | (ids if tie == "header" else np.uint64(0xFFFFFFFF) - ids)
    rank, most = _ranks(e["graph"], key)
    label = np.tile(np.arange(n, dtype=np.int64), (G, 1))
    in_msf = np.zeros(e["M"], np.int32)
    for j in range(most):
        at = np.flatnonzero(rank == j)
        g = e["graph"][at]
        a, b = label[g, e["lu"][at]], label[g, e["lv"][at]]
        take = a != b
        in_msf[at[take]] = 1
        g, a, b = g[take], a[take], b[take]
        rows = label[g]
        label[g] = np.where((rows == a[:, None]) | (rows == b[:, None]), np.maximum(a, b)[:, None], rows)
    components = int((label == np.arange(n)[None, :]).sum())
    e.update(in_msf=in_msf, comp=label, tree_edges=G * n - components, components=components)
    assert e["tree_edges"] == int(in_msf.sum())
    return e


def matching(A, val, numbering, heavy, seed, tie="header", ids="global", **broken):
    """The greedy matching in every graph at once: the edges in ascending MKEY = hi << 32 | lo, hi = k(weight) or its
    complement (heavy), lo = e or mix32(e ^ seed) (seed != 0) on the union's edge id e; an edge is kept when both its ends
    are free.  -> dict(mate (G, n) local, in_match (per edge), pairs, and the fields of edge_weights()).  tie = "larger"
    (lo = ~e under seed 0) and ids = "local" (lo from the edge's rank inside its graph) are wrong on purpose."""
    assert heavy in (0, 1)
    G, n, _ = A.shape
    e = edge_weights(A, val, numbering, **broken)
    eid = np.arange(e["M"], dtype=np.uint64)
    if ids == "local":
        eid = _ranks(e["graph"], eid)[0].astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFF
    lo = mix32(eid ^ np.uint64(seed)) if seed else (eid if tie == "header" else np.uint64(0xFFFFFFFF) - eid)
    hi = (e["k"] ^ np.uint32(0xFFFFFFFF) if heavy else e["k"]).astype(np.uint64)
    rank, most = _ranks(e["graph"], (hi << np.uint64(32)) | lo)
    mate = np.full((G, n), -1, np.int64)
    in_match = np.zeros(e["M"], np.int32)
    for j in range(most):
        at = np.flatnonzero(rank == j)
        g, u, v = e["graph"][at], e["lu"][at], e["lv"][at]
        take = (mate[g, u] < 0) & (mate[g, v] < 0)
        in_match[at[take]] = 1
        mate[g[take], u[take]], mate[g[take], v[take]] = v[take], u[take]
    e.update(mate=mate, in_match=in_match, pairs=int(in_match.sum()))
    return e


# ------------------------------------------------------------------ what the GPU file runs, and what the CPU file pins
UNIONS = (("digraphs", 3), ("digraphs", 4), ("undirected", 4), ("undirected", 5), ("undirected", 6))
COLOR_SETTINGS = tuple((order, seed, False) for order in (0, 1, 2) for seed in (0, 1)) + ((1, 1, True),)   # (order, seed, prio)
MATCH_SETTINGS = ((0, 0), (0, 1), (1, 0), (1, 1))                                                          # (heavy, seed)
RCM_UNIONS = (("undirected", 4), ("undirected", 5), ("digraphs", 3))
RCM_SETTINGS = ((0, 0), (0, 1), (8, 0), (8, 1))                                                            # (sweeps, reverse)


def graphs_of(kind, n):
    return all_digraphs(n) if kind == "digraphs" else all_undirected(n)


def storings(kind, A):
    """name -> mask of the entries written, for the weighted entry points: the digraphs as they are; the undirected
    graphs one way (halves) and both ways, where the smaller of two entries decides."""
    return {"as it is": None} if kind == "digraphs" else {"one way": halves(A), "both ways": None}


def color_schedule(A, depth):
    """(rounds, sizes, edges) of a complete sh_color run from the chain depths: round r's list is the vertices of depth r,
    its edges the sum of their degrees."""
    deg = simple(A).sum(axis=2)
    rounds = int(depth.max()) + 1
    return (rounds, np.bincount(depth.ravel(), minlength=rounds).astype(np.int64),
            np.bincount(depth.ravel(), weights=deg.ravel(), minlength=rounds).astype(np.int64))


# ------------------------------------------------------------------ telling a failure as a small graph
def picture(A, g):
    """Graph g as text: its bit pattern, n and local adjacency (row r lists the columns it stores)."""
    n = A.shape[1]
    rows = "; ".join(f"row {r} stores {np.flatnonzero(A[g, r]).tolist()}" for r in range(n))
    return f"graph g = {g} ({g:#x}), n = {n}: {rows} (an entry c in row r is the edge c -> r)"


def explain_vertices(A, numbering, want, got, ids_are_vertices=False, inputs=None, show=None):
    """'' when the two union vectors are equal, else the smallest graph with a differing vertex: its picture and the
    expected and actual local rows (union indices shown as local ones where they fall into the same graph), and the
    local rows of the union vectors in `inputs` (name -> vector: the sources, the start).  show(vector), if given, is what
    is printed of want and got (the floats behind the bits that were compared)."""
    want, got = np.asarray(want), np.asarray(got)
    if want.shape != got.shape:
        return f"shapes differ: expected {want.shape}, got {got.shape}"
    G, n, _ = A.shape
    bad = gather(want != got, G, n, numbering).any(axis=1)
    if not bad.any():
        return ""
    g = int(np.flatnonzero(bad)[0])
    ids = vertex_ids(G, n, numbering)[g]

    def row(vec):
        out = []
        for x in (vec if show is None else show(vec))[ids].tolist():
            if ids_are_vertices and x >= 0:
                at = np.flatnonzero(ids == x)
                x = int(at[0]) if len(at) else f"union vertex {x} of another graph"
            out.append(x)
        return out
    given = "".join(f"\n  {name} per local vertex: {np.asarray(vec)[ids].tolist()}" for name, vec in (inputs or {}).items())
    return (f"{int(bad.sum())} of {G} graphs differ; the smallest: {picture(A, g)}{given}\n"
            f"  expected per local vertex: {row(want)}\n  actual   per local vertex: {row(got)}")


def explain_edges(A, ref, want, got):
    """The same for a per-edge vector of the union; ref is truss()'s dict."""
    want, got = np.asarray(want), np.asarray(got)
    if want.shape != got.shape:
        return f"shapes differ: expected {want.shape}, got {got.shape}"
    bad = want != got
    if not bad.any():
        return ""
    g = int(ref["graph"][bad].min())
    mine = ref["graph"] == g
    ends = [f"{u}-{v}" for u, v in zip(ref["lu"][mine].tolist(), ref["lv"][mine].tolist())]
    return (f"{len(np.unique(ref['graph'][bad]))} graphs differ; the smallest: {picture(A, g)}\n  its edges (local ends): {ends}\n"
            f"  expected per edge: {want[mine].tolist()}\n  actual   per edge: {got[mine].tolist()}")
