"""Reference for sh_color (tests/test_color_ref.py pins it against the plain serial loop, the properties of a greedy
colouring and the host gold; tests/test_color_gpu.py compares the engine with it): schedule() is a model of the
Jones-Plassmann rounds -- the waiting counts, the list of every round, the marks taken in windows -- and gives the
colours with the records of the schedule (rounds, and size and edges per round), which are deterministic; first_fit() is
the plain serial first-fit in the order, the definition of the answer; mix32() is the tie of orders 1 and 2 in numpy.
The makers are those of the patterns the GPU tests run on.  No line here is shared with the product."""
import numpy as np

import core_ref as R
import tri_ref as T

SHORT, PIECE, WINDOW = 8, 2048, 32768   # the classes of the kernels (color.hip.h: GCOL_SHORT, GCOL_PIECE, GCOL_WINDOW)


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on 32-bit words (a bijection)."""
    x = np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def keys_of(n, deg, order, seed, prio=None, tie=None):
    """key[v] (a Python-sized integer per vertex, as int64): v precedes u exactly when key[v] > key[u].  The primary is
    prio when given, else the degree for order 2, else 0; the tie is `tie(v)` when given (for the broken rules of
    tests/test_color_ref.py), else the smaller index first for order 0 and the larger mix32(v ^ seed) first."""
    assert order in (0, 1, 2)
    v = np.arange(n, dtype=np.int64)
    primary = np.asarray(prio, np.int64)[:n] if prio is not None else (np.asarray(deg, np.int64) if order == 2 else np.zeros(n, np.int64))
    if tie is not None:
        low = np.asarray(tie(v), np.int64)
    elif order == 0:
        low = (1 << 32) - 1 - v
    else:
        low = mix32(v ^ (int(seed) & 0xFFFFFFFF)).astype(np.int64)
    return primary * (1 << 32) + low


def first_fit(n, rp, ci, va, order=0, seed=0, prio=None):
    """-> (color, colors, depth): the serial loop over the vertices in the order, each taking the smallest colour none of
    its coloured neighbours holds; depth[v] = the longest chain of preceding neighbours that ends in v, counted from 0."""
    ptr, col, deg, _ = R.lists_of(n, rp, ci, va)
    key = keys_of(n, deg, order, seed, prio)
    color, depth = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for v in np.argsort(-key, kind="stable").tolist():
        nb = col[ptr[v]:ptr[v + 1]]
        done = nb[color[nb] >= 0]
        held = set(color[done].tolist())
        c = 0
        while c in held:
            c += 1
        color[v] = c
        depth[v] = int(depth[done].max()) + 1 if len(done) else 0
    return color.astype(np.int32), (int(color.max()) + 1 if n else 0), depth.astype(np.int32)


def schedule(n, rp, ci, va, order=0, seed=0, prio=None, window=WINDOW, max_rounds=None, tie=None,
             decrement_coloured=False, every_walk_decrements=False, first_window_only=False):
    """-> dict(color, colors, rounds, complete, coloured, size, edges, wait, deg, M, max_degree).  wait[v] = the
    neighbours preceding v (as counted before round 0).  Round 0's list is the vertices with wait == 0; a round colours
    its whole list -- the marks of every vertex taken `window` colours at a time, a further walk per window while every
    colour of the window is held -- and takes one from the wait of every uncoloured neighbour per list vertex; those
    that reach 0 make the next list.  The last four parameters change the rule on purpose (tests/test_color_ref.py)."""
    ptr, col, deg, m = R.lists_of(n, rp, ci, va)
    key = keys_of(n, deg, order, seed, prio, tie)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    wait0 = np.bincount(row[key[col] > key[row]], minlength=n)[:n].astype(np.int64)
    wait, color = wait0.copy(), np.full(n, -1, np.int64)
    todo = np.flatnonzero(wait == 0)
    sizes, edges, complete, coloured = [], [], True, 0
    while coloured < n and len(todo):
        if max_rounds is not None and len(sizes) >= max_rounds:
            complete = False
            break
        seen = R._entries(ptr, col, todo)
        before = color.copy()   # (what a launch reads: no colour of this round)
        walks = np.ones(len(todo), np.int64)
        for i, v in enumerate(todo.tolist()):
            nb = col[ptr[v]:ptr[v + 1]]
            held = before[nb]
            held = held[held >= 0]
            size = min(window, len(held) + 1)   # (a free colour lies among the first len(held) + 1 of any run)
            lo = 0
            while True:
                marks = np.zeros(size, bool)
                if lo == 0 or not first_window_only:
                    marks[held[(held >= lo) & (held < lo + size)] - lo] = True
                if not marks.all():
                    color[v] = lo + int(np.argmin(marks))
                    break
                lo += window
                walks[i] += 1
        coloured += len(todo)
        sizes.append(len(todo))
        edges.append(len(seen))
        times = np.repeat(walks if every_walk_decrements else np.ones(len(todo), np.int64), ptr[todo + 1] - ptr[todo])
        keep = np.ones(len(seen), bool) if decrement_coloured else before[seen] < 0
        hits = np.bincount(seen[keep], weights=times[keep], minlength=n)[:n].astype(np.int64)
        wait -= hits
        todo = np.flatnonzero((hits > 0) & (wait == 0) & (color < 0))
    if coloured < n and complete and max_rounds is None:
        complete = False   # (only a broken rule gets here: vertices that nobody releases)
    return dict(color=color.astype(np.int32), colors=(int(color.max()) + 1 if n else 0), rounds=len(sizes), complete=complete,
                coloured=coloured, size=np.array(sizes, np.int64), edges=np.array(edges, np.int64), wait=wait0,
                deg=deg.astype(np.int32), M=m, max_degree=(int(deg.max()) if n else 0))


def is_proper(n, rp, ci, va, color):
    u, v = T.pairs_of(n, rp, ci, va)
    color = np.asarray(color)
    return bool((color[u] != color[v]).all())


# ---- the makers of the patterns (those of tri_ref / wcc_ref / core_ref where they exist)
def ear(k=5):
    """K_k with an ear: a path of three more vertices between two of the clique's."""
    a, b = np.triu_indices(k, 1)
    return T.from_pairs(k + 3, np.concatenate([a, [0, k, k + 1, k + 2]]), np.concatenate([b, [k, k + 1, k + 2, 1]]))


def wheel(n=12):
    """A rim of n vertices 1 .. n and the hub 0 tied to all of them."""
    rim = 1 + np.arange(n, dtype=np.int64)
    return T.from_pairs(n + 1, np.concatenate([np.zeros(n, np.int64), rim]), np.concatenate([rim, 1 + rim % n]))


def messy():
    """A small graph stored badly: self-loops, parallel entries, one-way entries, stored zeros, columns outside."""
    n, rp, ci, va = T.with_noise(*T.upper_only(*T.pattern(n=60, m=200, seed=5)))
    return n, rp, ci, va


def fan(L, k):
    """-> (n, rp, ci, va, hub, prio).  The hub is the vertex of the largest index, n - 1 = L, tied to all of 0 .. L - 1,
    so that entry i of its list is vertex i; k of those span a K_k: positions 0 and L - 1, positions 2047 and 2048 where
    the list is that long, the rest spread evenly; the other L - k are leaves.  prio puts the hub last (everything else
    precedes it): the leaves take colour 0, the clique 0 .. k - 1, and the hub's one walk -- by a lane, a wave or a
    workgroup -- has to see all of them to answer k."""
    assert 2 <= k <= L
    want = [0, L - 1] + [p for p in (PIECE - 1, PIECE) if 0 < p < L - 1]
    members = set(want)
    for p in np.linspace(0, L - 1, k).astype(np.int64).tolist() + list(range(L)):
        if len(members) == k:
            break
        members.add(int(p))
    mem = np.array(sorted(members), np.int64)
    x, y = np.triu_indices(k, 1)
    others = np.arange(L, dtype=np.int64)
    n, rp, ci, va = T.from_pairs(L + 1, np.concatenate([np.full(L, L, np.int64), mem[x]]), np.concatenate([others, mem[y]]))
    prio = np.zeros(n, np.int32)
    prio[L] = -1
    return n, rp, ci, va, L, prio


def fans(lengths, ks):
    """The disjoint union of fan(L, k) for the pairs of `lengths` and `ks` -> (n, rp, ci, va, hubs, prio)."""
    a, b, hubs, prios, base = [], [], [], [], 0
    for L, k in zip(lengths, ks):
        n, rp, ci, va, hub, prio = fan(L, k)
        u, v = T.pairs_of(n, rp, ci, va)
        a.append(base + u)
        b.append(base + v)
        hubs.append(base + hub)
        prios.append(prio)
        base += n
    n, rp, ci, va = T.from_pairs(base, np.concatenate(a), np.concatenate(b))
    return n, rp, ci, va, np.array(hubs, np.int64), np.concatenate(prios)
