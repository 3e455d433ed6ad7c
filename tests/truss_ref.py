"""Reference for sh_truss (tests/test_truss_ref.py pins it against a serial peel, the definition, the host gold and the
triangle total of tri_ref; tests/test_truss_gpu.py compares the engine with it): peel() is a set-based model of exactly
the schedule of csrc/truss.hip.h -- a stamp per edge, rounds, the tie-break by edge id between the two current edges of
a triangle, the clamp of the remaining support at the level's threshold s -- and returns the truss number and the
support of every edge with the records of the rounds (k, size, walked), which are deterministic.  serial() is the plain
peel, one edge at a time; holds_by_definition() the check straight from the definition; the makers are those of the
patterns the GPU tests run on that tri_ref / core_ref do not have.  No line here is shared with the product."""
import numpy as np

import tri_ref as T

SHORT, PIECE = 8, 2048   # the classes of the shorter list's length (truss.hip.h: TRUSS_SHORT, TRUSS_PIECE)
RULES = ("right", "double", "never", "keep-gone")   # the rule of the kernels and three deliberately broken ones


def graph_of(n, rp, ci, va):
    """-> (eu, ev, nb, ids): the edges of the simple undirected graph as the sorted unique pairs u < v (the index is the
    edge id), the neighbour sets, and the id of every pair as a dict keyed by u * n + v."""
    eu, ev = T.pairs_of(n, rp, ci, va)
    nb = [set() for _ in range(n)]
    for a, b in zip(eu.tolist(), ev.tolist()):
        nb[a].add(b)
        nb[b].add(a)
    ids = {a * n + b: i for i, (a, b) in enumerate(zip(eu.tolist(), ev.tolist()))}
    return eu, ev, nb, ids


def peel(n, rp, ci, va, max_rounds=None, rule="right"):
    """-> dict(truss, support, edge_u, edge_v, M, triangles, max_truss, levels, rounds, complete, k, size, walked).
    Round r walks the current edges (stamp == r): each is settled with truss = k = s + 2, and for every triangle
    {e, e1, e2} found from current e -- nothing if e1 or e2 is gone (0 < stamp < r) or both are current; if one is
    current the other is decremented by the smaller of the two current ids only; if neither is, both are.  A decrement
    applies only above s; the edge that reaches s is stamped r + 1 and makes the next list.  With an empty list the
    smallest remaining support among the unsettled becomes s and every unsettled edge that has it makes the list, in
    that same round.  rule != "right": a broken variant (test_truss_ref.py shows that the small graphs tell them apart)."""
    assert rule in RULES
    eu, ev, nb, ids = graph_of(n, rp, ci, va)
    m = len(eu)
    u_, v_ = eu.tolist(), ev.tolist()
    deg = [len(x) for x in nb]
    support = [len(nb[a] & nb[b]) for a, b in zip(u_, v_)]
    sup, stamp, truss = list(support), [0] * m, [0] * m
    todo, r, s, k, levels = [], 0, 0, 0, 0
    ks, sizes, walked = [], [], []
    remaining, complete = m, True

    def eid(a, b):
        return ids[a * n + b] if a < b else ids[b * n + a]

    while remaining > 0:
        if max_rounds is not None and r >= max_rounds:
            complete = False
            break
        r += 1
        if not todo:
            s = min(sup[e] for e in range(m) if stamp[e] == 0)
            k = s + 2
            todo = [e for e in range(m) if stamp[e] == 0 and sup[e] <= s]
            for e in todo:
                stamp[e] = r
            levels += 1
        nxt, w_sum = [], 0

        def dec(x):
            if sup[x] > s:
                sup[x] -= 1
                if sup[x] == s:
                    stamp[x] = r + 1
                    nxt.append(x)

        last = len(todo) == remaining   # every unsettled edge is current: no triangle has an edge left to decrement
        for e in todo:
            a, b = u_[e], v_[e]
            truss[e] = k
            w_sum += min(deg[a], deg[b])
            for w in (() if last and rule == "right" else nb[a] & nb[b]):
                e1, e2 = eid(a, w), eid(b, w)
                g1, g2 = 0 < stamp[e1] < r, 0 < stamp[e2] < r
                if g1 or g2:
                    if rule != "keep-gone":
                        continue
                    for x, g in ((e1, g1), (e2, g2)):   # (broken: the triangle is walked as if its gone edge were alive)
                        if not g and stamp[x] != r:
                            dec(x)
                    continue
                c1, c2 = stamp[e1] == r, stamp[e2] == r
                if c1 and c2:
                    continue
                if c1 or c2:
                    other, cur = (e2, e1) if c1 else (e1, e2)
                    if rule == "double" or (rule != "never" and e < cur):
                        dec(other)
                    continue
                dec(e1)
                dec(e2)
        ks.append(k)
        sizes.append(len(todo))
        walked.append(w_sum)
        remaining -= len(todo)
        todo = nxt
    total = sum(support)
    assert total % 3 == 0
    return dict(truss=np.array(truss, np.int32), support=np.array(support, np.int32), edge_u=eu.astype(np.int32),
                edge_v=ev.astype(np.int32), M=m, triangles=total // 3, max_truss=max(truss) if (m and ks) else 0,
                levels=levels, rounds=r, complete=complete, k=np.array(ks, np.int32), size=np.array(sizes, np.int64),
                walked=np.array(walked, np.int64))


def serial(n, rp, ci, va):
    """The truss numbers by the plain peel: the edge of the smallest remaining support leaves, alone, and takes one from
    the two other edges of every triangle it still closes."""
    eu, ev, nb, ids = graph_of(n, rp, ci, va)
    m = len(eu)
    u_, v_ = eu.tolist(), ev.tolist()
    sup = [len(nb[a] & nb[b]) for a, b in zip(u_, v_)]
    nb = [set(x) for x in nb]
    truss, k = [0] * m, 2
    buckets = {}
    for e, c in enumerate(sup):
        buckets.setdefault(c, set()).add(e)
    left, c = m, 0
    while left:
        c = min(x for x, b in buckets.items() if b) if not buckets.get(c) else c
        e = buckets[c].pop()
        k = max(k, c + 2)
        truss[e] = k
        left -= 1
        a, b = u_[e], v_[e]
        nb[a].discard(b)
        nb[b].discard(a)
        for w in nb[a] & nb[b]:
            for x, y in ((a, w), (b, w)):
                f = ids[x * n + y] if x < y else ids[y * n + x]
                buckets[sup[f]].discard(f)
                sup[f] -= 1
                buckets.setdefault(sup[f], set()).add(f)
                c = min(c, sup[f])
    return np.array(truss, np.int32)


def _peel_to(edges, nbr, need):
    """What is left of the edge set `edges` (ids) once every edge in fewer than `need` triangles of what is left has been
    deleted, again and again; nbr(e) -> the (e1, e2) pairs of e's triangles in the whole graph."""
    alive = set(edges)
    cnt = {e: sum(1 for e1, e2 in nbr(e) if e1 in alive and e2 in alive) for e in alive}
    todo = [e for e in alive if cnt[e] < need]
    while todo:
        nxt = []
        for e in todo:
            if e not in alive:
                continue
            alive.discard(e)
            for e1, e2 in nbr(e):
                if e1 in alive and e2 in alive:
                    for x in (e1, e2):
                        cnt[x] -= 1
                        if cnt[x] == need - 1:
                            nxt.append(x)
        todo = nxt
    return alive


def holds_by_definition(n, rp, ci, va, truss):
    """Is `truss` the vector of truss numbers, straight from the definition?  For every value k: (a) in the subgraph of
    the edges with truss >= k every edge lies in at least k - 2 triangles of it, so no value is too large to be
    reached; (b) no edge of truss k survives the peel of that subgraph at k + 1 (delete every edge in fewer than k - 1
    triangles until none is left), so no value is too small.  And no value is below 2."""
    eu, ev, nb, ids = graph_of(n, rp, ci, va)
    truss = np.asarray(truss, np.int64)
    if len(eu) == 0:
        return len(truss) == 0
    if len(truss) != len(eu) or truss.min() < 2:
        return False
    u_, v_ = eu.tolist(), ev.tolist()

    def eid(a, b):
        return ids[a * n + b] if a < b else ids[b * n + a]

    tris = [[(eid(a, w), eid(b, w)) for w in nb[a] & nb[b]] for a, b in zip(u_, v_)]
    nbr = tris.__getitem__
    for k in np.unique(truss).tolist():
        sub = set(np.flatnonzero(truss >= k).tolist())
        if _peel_to(sub, nbr, k - 2) != sub:                       # (a)
            return False
        left = _peel_to(sub, nbr, k - 1)
        if any(truss[e] == k for e in left):                       # (b)
            return False
    return True


# ---- the makers of the patterns that tri_ref / core_ref / wcc_ref do not have
def k5_ear():
    """K5 on 0..4 and vertex 5 tied to 0 and 1: truss 5 on the ten clique edges, 3 on the two ear edges."""
    a, b = np.triu_indices(5, 1)
    return T.from_pairs(6, np.concatenate([a, [0, 1]]), np.concatenate([b, [5, 5]]))


def k5_ear2():
    """k5_ear and vertex 6 tied to 1 and 5: truss 5 on the clique, 3 on the five other edges; {1, 5} is settled one round
    after {0, 5}."""
    a, b = np.triu_indices(5, 1)
    return T.from_pairs(7, np.concatenate([a, [0, 1, 1, 5]]), np.concatenate([b, [5, 5, 6, 6]]))


def two_hubs(L):
    """Vertices 0 and 1 tied, and both tied to L leaves: every truss is 3, support{0, 1} = L, two rounds of sizes 2L and
    1; the shorter list of the hub edge has L + 1 entries."""
    leaves = 2 + np.arange(L, dtype=np.int64)
    return T.from_pairs(L + 2, np.concatenate([[0], np.zeros(L, np.int64), np.ones(L, np.int64)]),
                        np.concatenate([[1], leaves, leaves]))


def hub_pair(L, where):
    """Hubs u and v tied, each with L leaves of its own and one common neighbour w; {u, w} lies in a K5 with three
    further vertices and {v, w} in another.  Truss 2 on the 2L leaf edges, 3 on {u, v}, 5 on the twenty clique edges.
    where: w is the "first", a "middle" or the "last" entry of both hubs' lists (which hold L + 5 entries each).
    -> (n, rp, ci, va, (u, v, w))"""
    half = L // 2
    if where == "first":
        w, u, v, base = 0, 1, 2, 3
        lu = base + np.arange(L, dtype=np.int64)
        lv = base + L + np.arange(L, dtype=np.int64)
        extra = base + 2 * L + np.arange(6, dtype=np.int64)
    elif where == "last":
        u, v, base = 0, 1, 2
        lu = base + np.arange(L, dtype=np.int64)
        lv = base + L + np.arange(L, dtype=np.int64)
        extra = base + 2 * L + np.arange(6, dtype=np.int64)
        w = base + 2 * L + 6
    else:
        assert where == "middle"
        u, v, base = 0, 1, 2
        lo = base + np.arange(2 * half, dtype=np.int64)               # the leaves below w ...
        w = base + 2 * half
        extra = w + 1 + np.arange(6, dtype=np.int64)
        hi = w + 7 + np.arange(2 * (L - half), dtype=np.int64)        # ... and those above
        lu = np.concatenate([lo[:half], hi[:L - half]])
        lv = np.concatenate([lo[half:], hi[L - half:]])
    n = 2 * L + 9
    ka, kb = np.array([u, w, *extra[:3]], np.int64), np.array([v, w, *extra[3:]], np.int64)
    p, q = np.triu_indices(5, 1)
    a = np.concatenate([[u], np.full(L, u, np.int64), np.full(L, v, np.int64), ka[p], kb[p]])
    b = np.concatenate([[v], lu, lv, ka[q], kb[q]])
    return T.from_pairs(n, a, b) + ((u, v, w),)
