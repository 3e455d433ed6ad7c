"""Reference for sh_rcm (tests/test_rcm_ref.py pins it: the serial loop against the level-synchronous simulator, both
against certify(), the host gold and brute-force bandwidth and profile; tests/test_rcm_gpu.py compares the engine with
it): serial() is the definition of the answer, one queue and one vertex at a time; levels() reproduces it level by level
-- every vertex of the next level goes to the smallest position of the current level adjacent to it, every position
emits the entries of its list that it owns in list order -- and gives the records of the schedule (one step per level of
every breadth-first search), which are deterministic; certify() checks a permutation without any gold.  The makers are
those of the patterns the GPU tests run on.  No line here is shared with the product."""
import numpy as np

import core_ref as R
import tri_ref as T
import wcc_ref as W

LANE, WAVE = 8, 2048   # the list-walk tiers of the kernels (rcm.hip.h: RCM_LANE, RCM_WAVE)
BATCHES = (8, 16, 32)  # run_batches: the first batch holds 8 steps, the next ones twice as many up to RCM_BATCH = 32


def graph_of(n, rp, ci, va):
    """-> (ptr, col, deg, M, rank): the symmetric lists, each sorted by ascending (deg, index); rank[v] = the place of v
    in the ascending (deg, index) order of all vertices (so "smaller" is the smaller rank)."""
    ptr, col, deg, m = R.lists_of(n, rp, ci, va)
    rank = np.empty(n, np.int64)
    rank[np.lexsort((np.arange(n), deg))] = np.arange(n)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = col[np.lexsort((rank[col], row))]
    return ptr, col, deg, m, rank


def _search(ptr, col, rank, src):
    """A breadth-first search from src -> (eccentricity, the smallest vertex of its last level, widths, list entries)."""
    seen = {src}
    level, widths, looked = [src], [], []
    while True:
        widths.append(len(level))
        looked.append(int(sum(ptr[v + 1] - ptr[v] for v in level)))
        nxt = []
        for v in level:
            for w in col[ptr[v]:ptr[v + 1]].tolist():
                if w not in seen:
                    seen.add(w)
                    nxt.append(w)
        if not nxt:
            return len(widths) - 1, min(level, key=lambda v: rank[v]), widths, looked
        level = nxt


def _root(ptr, col, rank, v, sweeps):
    """George and Liu with a cap -> (r, searches): the records of every search run, in order."""
    if sweeps == 0:
        return v, []
    e, x, widths, looked = _search(ptr, col, rank, v)
    r, runs = v, [(widths, looked)]
    for _ in range(sweeps):
        if x == r:
            break
        e2, x2, widths, looked = _search(ptr, col, rank, x)
        runs.append((widths, looked))
        if e2 <= e:
            break
        r, e, x = x, e2, x2
    return r, runs


def serial(n, rp, ci, va, sweeps=8, reverse=1):
    """-> dict(perm, pos, level, components, roots): the definition.  One queue, one vertex at a time."""
    ptr, col, deg, m, rank = graph_of(n, rp, ci, va)
    pos, level, order, roots = np.full(n, -1, np.int64), np.full(n, -1, np.int64), [], []
    for v in np.argsort(rank).tolist():
        if pos[v] >= 0:
            continue
        r = v if deg[v] == 0 else _root(ptr, col, rank, v, sweeps)[0]
        roots.append(r)
        head = len(order)
        pos[r], level[r] = len(order), 0
        order.append(r)
        while head < len(order):
            u = order[head]
            head += 1
            for w in col[ptr[u]:ptr[u + 1]].tolist():
                if pos[w] < 0:
                    pos[w], level[w] = len(order), level[u] + 1
                    order.append(w)
    if reverse:
        pos = n - 1 - pos
    perm = np.empty(n, np.int64)
    perm[pos] = np.arange(n)
    return dict(perm=perm.astype(np.int32), pos=pos.astype(np.int32), level=level.astype(np.int32), components=len(roots),
                roots=np.array(roots, np.int64))


def levels(n, rp, ci, va, sweeps=8, reverse=1, max_steps=None, owner="smallest", emit="list"):
    """-> dict(perm, pos, level, components, sweeps_run, steps, complete, kind, size, edges, bandwidth_before,
    bandwidth_after, profile_before, profile_after, M, max_degree, roots).  The schedule of the device: a step is one
    level of one search; kind 0 for a root search, 1 for the numbering.  After max_steps steps the run stops: the
    numbered part of perm is as the full run gives it, the rest -1, and both values after are -1.  `owner` and `emit`
    change the rule on purpose (tests/test_rcm_ref.py): owner = "largest" gives a vertex to the largest adjacent position,
    emit = "index" emits a position's children in ascending index instead of list order."""
    ptr, col, deg, m, rank = graph_of(n, rp, ci, va)
    pos, level, order, roots = np.full(n, -1, np.int64), np.full(n, -1, np.int64), [], []
    kind, size, edges = [], [], []
    components = sweeps_run = 0
    cap = max_steps if max_steps is not None else (sweeps + 2) * n + 1

    class Cut(Exception):
        pass

    def step(k, width, looked):
        if len(kind) >= cap:
            raise Cut
        kind.append(k)
        size.append(width)
        edges.append(looked)

    try:
        for v in np.argsort(rank).tolist():
            if pos[v] >= 0:
                continue
            if deg[v] == 0:
                pos[v], level[v] = len(order), 0
                order.append(v)
                roots.append(v)
                components += 1
                continue
            r, runs = _root(ptr, col, rank, v, sweeps)
            for widths, looked in runs:
                for a, b in zip(widths, looked):
                    step(0, a, b)
                sweeps_run += 1
            roots.append(r)   # (the step that ends the last search also gives r its position)
            pos[r], level[r] = len(order), 0
            order.append(r)
            a, b, lvl = len(order) - 1, len(order), 0
            while True:
                step(1, b - a, int(sum(ptr[order[i] + 1] - ptr[order[i]] for i in range(a, b))))
                own = {}
                for i in range(a, b):
                    for w in col[ptr[order[i]]:ptr[order[i] + 1]].tolist():
                        if pos[w] < 0:
                            own[w] = min(own.get(w, i), i) if owner == "smallest" else max(own.get(w, i), i)
                for i in range(a, b):
                    mine = [w for w in col[ptr[order[i]]:ptr[order[i] + 1]].tolist() if own.get(w) == i]
                    for w in (mine if emit == "list" else sorted(mine)):
                        pos[w], level[w] = len(order), lvl + 1
                        order.append(w)
                if len(order) == b:
                    break
                a, b, lvl = b, len(order), lvl + 1
            components += 1
        complete = True
    except Cut:
        complete = False
    done = len(order)
    p = np.where(pos >= 0, n - 1 - pos, -1) if reverse else pos.copy()
    perm = np.full(n, -1, np.int64)
    perm[p[p >= 0]] = np.flatnonzero(p >= 0)
    bw0, prof0 = spread(n, rp, ci, va, np.arange(n))
    bw1, prof1 = spread(n, rp, ci, va, p) if complete else (-1, -1)
    return dict(perm=perm.astype(np.int32), pos=p.astype(np.int32), level=level.astype(np.int32), components=components,
                sweeps_run=sweeps_run, steps=len(kind), complete=complete, kind=np.array(kind, np.int32),
                size=np.array(size, np.int64), edges=np.array(edges, np.int64), bandwidth_before=bw0, bandwidth_after=bw1,
                profile_before=prof0, profile_after=prof1, M=m, max_degree=(int(deg.max()) if n else 0),
                roots=np.array(roots, np.int64), done=done)


def spread(n, rp, ci, va, p):
    """-> (bandwidth, profile) of the simple graph under positions p: max |p(u) - p(v)| over the edges, and the sum over
    v of p(v) - min(p(v), min over the neighbours u of p(u))."""
    u, v = T.pairs_of(n, rp, ci, va)
    p = np.asarray(p, np.int64)
    if len(u) == 0:
        return 0, 0
    first = p.copy()
    np.minimum.at(first, u, p[v])
    np.minimum.at(first, v, p[u])
    return int(np.abs(p[u] - p[v]).max()), int((p - first).sum())


def certify(n, rp, ci, va, perm, roots, reverse=1):
    """None when perm is a Cuthill-McKee order (reversed when `reverse`) of the graph with the given roots, else the
    first rule it breaks.  Needs no gold: perm is a permutation; every component is a contiguous range that starts with
    its root; first[v] (the smallest position of a neighbour) is below pos[v] for every vertex but a root; first is
    non-decreasing along a component; vertices with equal first ascend in (deg, index)."""
    ptr, col, deg, m, rank = graph_of(n, rp, ci, va)
    perm = np.asarray(perm, np.int64)
    if len(perm) != n or sorted(perm.tolist()) != list(range(n)):
        return "perm is no permutation"
    order = perm[::-1] if reverse else perm
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    comp = W.components(n, rp, ci, va)
    roots = set(int(r) for r in roots)
    k = 0
    while k < n:
        members = np.flatnonzero(comp == comp[order[k]])
        if sorted(order[k:k + len(members)].tolist()) != members.tolist():
            return f"the component at position {k} is no contiguous range"
        if int(order[k]) not in roots:
            return f"position {k} starts a component with a vertex that is no root"
        last = None
        for i in range(k + 1, k + len(members)):
            v = order[i]
            first = int(pos[col[ptr[v]:ptr[v + 1]]].min())
            if first >= i:
                return f"position {i}: no neighbour stands before it"
            if last is not None and first < last[0]:
                return f"position {i}: first decreases"
            if last is not None and first == last[0] and rank[v] < last[1]:
                return f"position {i}: equal first, but (deg, index) descends"
            last = (first, rank[v])
        k += len(members)
    return None


# ---- the makers of the patterns
def empty(n):
    return n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def graph_k(k, mask):
    """The pairs of the graph on k labelled vertices whose edge i (in the order of the pairs u < v) is present when bit i
    of mask is set."""
    pairs = [(u, v) for u in range(k) for v in range(u + 1, k)]
    return [pr for i, pr in enumerate(pairs) if mask >> i & 1]


def small(k, mask):
    have = graph_k(k, mask)
    return T.from_pairs(k, [u for u, v in have], [v for u, v in have])


def union(parts):
    """The disjoint union of (n, pairs) parts -> CSR arrays."""
    a, b, base = [], [], 0
    for n, pairs in parts:
        a += [base + u for u, v in pairs]
        b += [base + v for u, v in pairs]
        base += n
    return T.from_pairs(base, np.array(a, np.int64), np.array(b, np.int64))


def all_graphs4():
    """All 64 graphs on 4 labelled vertices in one matrix: many components, ties, and roots that move."""
    return union([(4, graph_k(4, mask)) for mask in range(64)])


def stars(leaves, path=40):
    """Stars of the given numbers of leaves (the hub first) beside a path."""
    parts = [(k + 1, [(0, i) for i in range(1, k + 1)]) for k in leaves]
    parts.append((path, [(i, i + 1) for i in range(path - 1)]))
    return union(parts)


def broom(k=300_001):
    """A hub (vertex 0) with k leaves 1 .. k, each carrying one pendant k + 1 .. 2k."""
    leaf = np.arange(1, k + 1, dtype=np.int64)
    return T.from_pairs(2 * k + 1, np.concatenate([np.zeros(k, np.int64), leaf]), np.concatenate([leaf, leaf + k]))


def shuffled(mat, seed=5):
    """The same graph with its vertices relabelled by a seeded permutation."""
    n, rp, ci, va = mat
    name = np.random.default_rng(seed).permutation(n)
    u, v = T.pairs_of(n, rp, ci, va)
    return T.from_pairs(n, name[u], name[v])


def drawn(n, m, seed):
    """m drawn pairs on n vertices (loops and repeats included: the cleaning drops them)."""
    rng = np.random.default_rng(seed)
    return T.from_pairs(n, rng.integers(0, n, m), rng.integers(0, n, m))
