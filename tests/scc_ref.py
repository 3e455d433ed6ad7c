"""References for sh_scc (tests/test_scc_ref.py pins them, tests/test_scc_gpu.py compares the engine with them):
components() is Tarjan's algorithm written out iteratively, schedule() a numpy model of the engine's fixed schedule
(include/sparseharness_hip.h: trim round, one pivot round, colouring rounds), and three pattern makers whose components
or round counts are known by construction."""
import numpy as np


def edges_of(n, rp, ci, va):
    """-> (src, dst): entry (r, c) is the edge c -> r when 0 <= c < n and its 32 value bits are not all zero."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    bits = np.ascontiguousarray(va).view(np.uint32)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = (ci >= 0) & (ci < n) & (bits != 0)
    return ci[keep], rows[keep]


def components(n, rp, ci, va):
    """comp[v] = the largest vertex index of v's strongly connected component (iterative Tarjan)."""
    src, dst = edges_of(n, rp, ci, va)
    order = np.argsort(src, kind="stable")
    adj = dst[order].tolist()
    ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).tolist()
    index, low, on = [-1] * n, [0] * n, [False] * n
    nxt = ptr[:n]
    comp = np.full(n, -1, np.int64)
    stack, count = [], 0
    for root in range(n):
        if index[root] != -1:
            continue
        index[root] = low[root] = count
        count += 1
        stack.append(root)
        on[root] = True
        path = [root]
        while path:
            v = path[-1]
            if nxt[v] < ptr[v + 1]:
                c = adj[nxt[v]]
                nxt[v] += 1
                if index[c] == -1:
                    index[c] = low[c] = count
                    count += 1
                    stack.append(c)
                    on[c] = True
                    path.append(c)
                elif on[c]:
                    low[v] = min(low[v], index[c])
                continue
            path.pop()
            if path:
                low[path[-1]] = min(low[path[-1]], low[v])
            if low[v] == index[v]:
                at = len(stack) - 1
                while stack[at] != v:
                    at -= 1
                members = stack[at:]
                del stack[at:]
                top = max(members)
                for u in members:
                    on[u] = False
                    comp[u] = top
    return comp.astype(np.int32)


def _reach(n, src, dst, start):
    """The vertices `start` (a boolean vector) reaches along the edges src -> dst, itself included."""
    seen = start.copy()
    while True:
        hit = np.zeros(n, bool)
        hit[dst[seen[src]]] = True
        hit &= ~seen
        if not hit.any():
            return seen
        seen |= hit


def schedule(n, rp, ci, va, trim, pivot):
    """-> (comp, kinds, sizes): the engine's schedule, round by round.  kinds: 0 trim, 1 pivot, 2 colouring; sizes: the
    vertices each round settled.  A trim round that settles nothing is not recorded."""
    src, dst = edges_of(n, rp, ci, va)
    in_len, out_len = np.bincount(dst, minlength=n).astype(np.uint64), np.bincount(src, minlength=n).astype(np.uint64)
    loop = src == dst
    src, dst = src[~loop], dst[~loop]          # self-loops never count
    comp = np.full(n, -1, np.int64)
    kinds, sizes = [], []
    pivot_done = False
    ids = np.arange(n, dtype=np.int64)
    while (comp < 0).any():
        live = comp < 0
        keep = live[src] & live[dst]           # edges count only between live vertices
        src, dst = src[keep], dst[keep]
        if trim:
            gone = 0
            while True:
                live = comp < 0
                keep = live[src] & live[dst]
                src, dst = src[keep], dst[keep]
                die = live & ((np.bincount(dst, minlength=n) == 0) | (np.bincount(src, minlength=n) == 0))
                if not die.any():
                    break
                comp[die] = ids[die]
                gone += int(die.sum())
            if gone:
                kinds.append(0)
                sizes.append(gone)
            live = comp < 0
            if not live.any():
                break
        if pivot and not pivot_done:
            pivot_done = True
            prod = np.where(live, in_len * out_len, 0)
            best = prod[live].max()
            p = int(ids[live & (prod == best)].max())
            start = np.zeros(n, bool)
            start[p] = True
            fwd = _reach(n, src, dst, start)
            inside = fwd[src] & fwd[dst]
            claimed = _reach(n, dst[inside], src[inside], start)
            comp[claimed] = ids[claimed].max()
            kinds.append(1)
            sizes.append(int(claimed.sum()))
            continue
        colour = np.where(live, ids, -1)
        order = np.argsort(dst, kind="stable")
        s_src, s_dst = src[order], dst[order]
        heads, first = np.unique(s_dst, return_index=True)
        while len(heads):                       # colour[u] = the largest live index that reaches u
            best = np.maximum.reduceat(colour[s_src], first)
            new = colour.copy()
            new[heads] = np.maximum(new[heads], best)
            if np.array_equal(new, colour):
                break
            colour = new
        roots = live & (colour == ids)
        same = colour[src] == colour[dst]       # a claim follows an edge c -> v only where colour[c] == colour[v]
        claimed = _reach(n, dst[same], src[same], roots)
        comp[claimed] = colour[claimed]
        kinds.append(2)
        sizes.append(int(claimed.sum()))
    return comp.astype(np.int32), kinds, sizes


def _csr(n, src, dst, va=None):
    """Edges src -> dst as the CSR arrays of the matrix that stores them (row = dst, column = src), values 1.0."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.lexsort((src, dst))
    rp = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    va = np.ones(len(src), np.float32) if va is None else np.asarray(va, np.float32)[order]
    return rp, src[order].astype(np.int32), va


PLANTED_BLOCKS = (1, 1, 2, 3, 8, 9, 64, 65, 300)


def planted(seed=3):
    """-> (n, rp, ci, va, want).  Blocks of PLANTED_BLOCKS vertices, each a directed cycle plus random chords; edges between
    blocks go only forwards in a random block order; vertex indices shuffled; stored zeros and out-of-range columns laid
    over it (neither is an edge).  The components are the blocks, by construction: want[v] = the largest index of v's."""
    rng = np.random.default_rng(seed)
    n = sum(PLANTED_BLOCKS)
    name = rng.permutation(n)                    # vertex k of the construction is called name[k]
    block_order = rng.permutation(len(PLANTED_BLOCKS))
    starts = np.concatenate([[0], np.cumsum(PLANTED_BLOCKS)])
    src, dst, block_of = [], [], np.zeros(n, np.int64)
    for b, size in enumerate(PLANTED_BLOCKS):
        lo = starts[b]
        block_of[lo:lo + size] = b
        if size > 1:
            src.append(lo + np.arange(size))
            dst.append(lo + (np.arange(size) + 1) % size)
            src.append(lo + rng.integers(0, size, size))
            dst.append(lo + rng.integers(0, size, size))
    rank = np.empty(len(PLANTED_BLOCKS), np.int64)
    rank[block_order] = np.arange(len(PLANTED_BLOCKS))
    a, b = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    fwd = rank[block_of[a]] < rank[block_of[b]]
    src.append(a[fwd])
    dst.append(b[fwd])
    src, dst = name[np.concatenate(src)], name[np.concatenate(dst)]
    va = np.ones(len(src), np.float32)
    # noise that is no edge: stored zeros anywhere (backwards too), columns outside the matrix
    zs, zd = rng.integers(0, n, n), rng.integers(0, n, n)
    os_, od = np.where(rng.random(60) < 0.5, -1 - rng.integers(0, 4, 60), n + rng.integers(0, 50, 60)), rng.integers(0, n, 60)
    src = np.concatenate([src, zs, os_])
    dst = np.concatenate([dst, zd, od])
    va = np.concatenate([va, np.zeros(n, np.float32), np.ones(60, np.float32)])
    rp, ci, va = _csr(n, src, dst, va)
    want = np.empty(n, np.int32)
    for b, size in enumerate(PLANTED_BLOCKS):
        members = name[starts[b]:starts[b] + size]
        want[members] = members.max()
    return n, rp, ci, va, want


def cycle_chain(k=12, length=20, descending=True):
    """-> (n, rp, ci, va).  k directed cycles of `length` vertices, cycle i on the vertices [i * length, (i + 1) * length),
    one edge from each cycle to the next.  descending: the chain runs from the cycle with the largest indices down, so
    the largest live index colours everything below it and a colouring round settles ONE cycle: k rounds.  Ascending:
    every cycle keeps its own largest index as colour: one round."""
    n = k * length
    v = np.arange(n, dtype=np.int64)
    src, dst = [v], [(v // length) * length + (v % length + 1) % length]
    a, b = np.arange(k - 1, dtype=np.int64) * length, np.arange(1, k, dtype=np.int64) * length
    src.append(b if descending else a)
    dst.append(a if descending else b)
    return (n,) + _csr(n, np.concatenate(src), np.concatenate(dst))


def path(n=500):
    """-> (n, rp, ci, va): the directed path n - 1 -> n - 2 -> ... -> 0.  Trim settles everything; without trim the
    largest live index colours all that is left and a colouring round settles that one vertex: n rounds."""
    v = np.arange(n - 1, dtype=np.int64)
    return (n,) + _csr(n, v + 1, v)
