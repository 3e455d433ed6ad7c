"""Reference for sh_core (tests/test_core_ref.py pins it against an independent method, the definition, closed forms and
the host gold; tests/test_core_gpu.py compares the engine with it): peel() gives the core number of every vertex of the
simple undirected graph under a CSR pattern by peeling synchronously, round by round, and with them the records of the
schedule with chase == 0 (rounds, levels, and k, size and edges per round), which are deterministic.  hindex() is the
independent method, holds_by_definition() the check straight from the definition, and the makers are those of the
patterns the GPU tests run on.  No line here is shared with the product."""
import numpy as np

import tri_ref as T
import wcc_ref as W

SHORT, PIECE = 8, 2048   # the list-length classes of the kernels (core.hip.h: CORE_SHORT, CORE_PIECE)


def lists_of(n, rp, ci, va):
    """-> (ptr, col, deg, M): the symmetric neighbour lists of the simple undirected graph, ascending."""
    u, v = T.pairs_of(n, rp, ci, va)
    src, dst = np.concatenate([u, v]), np.concatenate([v, u])
    order = np.lexsort((dst, src))
    deg = np.bincount(src, minlength=n)[:n].astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return ptr, dst[order].astype(np.int64), deg, len(u)


def _entries(ptr, col, verts):
    """The list entries of `verts`, all in one array."""
    lens = ptr[verts + 1] - ptr[verts]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    starts = np.repeat(ptr[verts] - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return col[starts + np.arange(total, dtype=np.int64)]


def peel(n, rp, ci, va, max_rounds=None):
    """-> dict(core, deg, M, degeneracy, levels, rounds, complete, k, size, edges).  A round settles its whole work list
    at level k and takes one from the remaining degree of every unsettled neighbour per settled neighbour, never below
    k; the vertices that reach k make the next list.  With an empty list the smallest remaining degree among the
    unsettled becomes k and every unsettled vertex that has it makes the list, in that same round."""
    ptr, col, deg, m = lists_of(n, rp, ci, va)
    cur, core = deg.copy(), np.full(n, -1, np.int64)
    todo = np.zeros(0, np.int64)
    k, levels, ks, sizes, edges = 0, 0, [], [], []
    remaining, complete = n, True
    while remaining > 0:
        if max_rounds is not None and len(ks) >= max_rounds:
            complete = False
            break
        if len(todo) == 0:
            open_ = core < 0
            k = int(cur[open_].min())
            todo = np.flatnonzero(open_ & (cur <= k))
            levels += 1
        core[todo] = k
        remaining -= len(todo)
        seen = _entries(ptr, col, todo)
        ks.append(k)
        sizes.append(len(todo))
        edges.append(len(seen))
        hits = np.bincount(seen, minlength=n)[:n]
        live = (cur > k) & (hits > 0)
        cur[live] = np.maximum(cur[live] - hits[live], k)
        todo = np.flatnonzero(live & (cur <= k))
    return dict(core=core.astype(np.int32), deg=deg.astype(np.int32), M=m, degeneracy=max(k if ks else 0, 0), levels=levels,
                rounds=len(ks), complete=complete, k=np.array(ks, np.int32), size=np.array(sizes, np.int64),
                edges=np.array(edges, np.int64))


def hindex(n, rp, ci, va, max_iters=1 << 20):
    """The core numbers by another road (Lu, Lai, Chen, Zhou, Zhang, Stanley, "The H-index of a network node and its
    relation to degree and coreness", Nature Communications 2016): start from the degrees and replace every value by the
    H-index of its neighbours' values until nothing changes."""
    ptr, col, deg, _ = lists_of(n, rp, ci, va)
    h = deg.copy()
    if len(col) == 0:
        return h.astype(np.int32)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    rank = np.arange(len(col), dtype=np.int64) - ptr[row] + 1      # 1, 2, ... inside every list
    for _ in range(max_iters):
        order = np.lexsort((-h[col], row))                         # every list by value, descending
        ok = h[col][order] >= rank                                 # the i-th largest is at least i
        new = np.bincount(row[ok], minlength=n)[:n]
        if np.array_equal(new, h):
            return h.astype(np.int32)
        h = new
    raise AssertionError("the H-index iteration did not converge")


def holds_by_definition(n, rp, ci, va, core):
    """Is `core` the vector of core numbers, straight from the definition?  (a) Every v has at least core[v] neighbours
    u with core[u] >= core[v]: the vertices of core >= c span a subgraph of minimum degree >= c, so no value is too
    large to be reached.  (b) For every value k: after deleting all vertices with core < k, no vertex of core >= k + 1
    has degree < k + 1 among those of core >= k, and the vertices of core == k can be deleted in waves, each vertex
    with at most k neighbours left when it goes: none of them lies in a subgraph of minimum degree k + 1, so no value
    is too small.  (c) Deleting the vertices of core < k for k = core.max() + 1 leaves nothing."""
    ptr, col, deg, _ = lists_of(n, rp, ci, va)
    core = np.asarray(core, np.int64)
    if n == 0:
        return True
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    up = np.bincount(row[core[col] >= core[row]], minlength=n)[:n]
    if not (up >= core).all():                                     # (a)
        return False
    for k in np.unique(core).tolist():
        # the graph left when everything with core < k is gone; its vertices of core == k must peel away at degree <= k
        alive = core >= k
        left = np.bincount(row[alive[row] & alive[col]], minlength=n)[:n]
        if (left[core >= k + 1] < k + 1).any():
            return False
        level = alive & (core == k)
        gone = np.zeros(n, bool)
        while True:
            ready = level & ~gone & (left <= k)
            if not ready.any():
                break
            gone |= ready
            hit = _entries(ptr, col, np.flatnonzero(ready))
            left = left - np.bincount(hit, minlength=n)[:n]
        if (level & ~gone).any():                                  # (b): a vertex of core k that does not peel at k
            return False
    return not (core >= core.max() + 1).any()                      # (c)


# ---- the makers of the patterns (those of tri_ref / wcc_ref where they exist)
def star(k):
    return T.from_pairs(k + 1, np.zeros(k, np.int64), 1 + np.arange(k, dtype=np.int64))


def cycle(n):
    v = np.arange(n, dtype=np.int64)
    return T.from_pairs(n, v, (v + 1) % n)


def tree(n=3001, seed=9):
    return W.one_way(n, seed=seed)


def cliques(lo=2, hi=40):
    """The disjoint union of K_lo ... K_hi: core n - 1 on K_n, hi - lo + 1 levels."""
    a, b, base = [], [], 0
    for n in range(lo, hi + 1):
        x, y = np.triu_indices(n, 1)
        a.append(base + x)
        b.append(base + y)
        base += n
    return T.from_pairs(base, np.concatenate(a), np.concatenate(b))


def isolated(n=100, extra=7):
    """A cycle of n vertices and `extra` vertices alone."""
    c = cycle(n)
    return T.from_pairs(n + extra, *T.pairs_of(*c))


HUB_DEGREES = (SHORT, SHORT + 1, PIECE, PIECE + 1, 2 * PIECE + 1)


def class_limits():
    """One hub per degree d of HUB_DEGREES whose list is walked while it still has unsettled neighbours, and whose
    decrements decide their core numbers.  Block: the hub, x, a K_4, d - 2 pendant leaves, y, in index order (so x
    stands in the first piece of the hub's list and y in the last).  The hub is tied to the leaves, x and y; x to two
    vertices of the K_4 and y to the other two.  Level 1 takes the leaves (each decrements the hub, which stays at 2).
    Level 2 opens with the hubs alone (x and y stand at 3, the K_4 at 4): the hub's whole list of d entries is walked --
    by one lane, one wave or in pieces -- and its decrements bring x and y to 2, so they fall at level 2.  A walk that
    missed one would leave it at 3 and settle it with the K_4 at level 3.  core: leaves 1, hubs, x and y 2, the K_4s 3."""
    a, b, base, hubs = [], [], 0, []
    for d in HUB_DEGREES:
        hub, x, k4 = base, base + 1, base + 2 + np.arange(4, dtype=np.int64)
        leaves = base + 6 + np.arange(d - 2, dtype=np.int64)
        y = base + 6 + d - 2
        p, q = np.triu_indices(4, 1)
        a += [np.full(d - 2, hub, np.int64), np.array([hub, hub, x, x, y, y], np.int64), k4[p]]
        b += [leaves, np.array([x, y, k4[0], k4[1], k4[2], k4[3]], np.int64), k4[q]]
        hubs.append(hub)
        base = y + 1
    n, rp, ci, va = T.from_pairs(base, np.concatenate(a), np.concatenate(b))
    return n, rp, ci, va, np.array(hubs, np.int64)


def big_hub(k=70_001, clique=0):
    """A hub of k pendant leaves (core 1 everywhere); with clique = c > 0 the hub also belongs to a K_c (the hub and
    c - 1 more vertices): the hub and they have core c - 1."""
    a, b = [np.zeros(k, np.int64)], [1 + np.arange(k, dtype=np.int64)]
    n = k + 1
    if clique:
        members = np.concatenate([[0], n + np.arange(clique - 1, dtype=np.int64)])
        x, y = np.triu_indices(clique, 1)
        a.append(members[x])
        b.append(members[y])
        n += clique - 1
    return T.from_pairs(n, np.concatenate(a), np.concatenate(b))
