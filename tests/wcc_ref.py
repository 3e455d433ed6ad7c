"""Reference for sh_wcc (tests/test_wcc_ref.py pins it, tests/test_wcc_gpu.py compares the engine with it): components()
is a union-find over scc_ref.edges_of's edges taken both ways, and the makers of the patterns the GPU tests run on, whose
components are known by construction or are checked against the reference there."""
import numpy as np

import scc_ref as S

SHORT, PIECE = 8, 2048   # the list-length classes of the kernels (wcc.hip.h: WCC_SHORT, WCC_PIECE)


def components(n, rp, ci, va):
    """comp[v] = the largest vertex index of v's weakly connected component.  Union-find in numpy: every round points
    each root at the largest root one of its edges leads to, then flattens by pointer doubling."""
    src, dst = S.edges_of(n, rp, ci, va)
    p = np.arange(n, dtype=np.int64)
    while True:
        a, b = p[src], p[dst]
        live = a != b
        if not live.any():
            return p.astype(np.int32)
        a, b = a[live], b[live]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        np.maximum.at(p, lo, hi)              # roots only: p is flat here, so lo and hi are roots
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q


def csr(n, src, dst, va=None):
    """Edges src -> dst as CSR arrays (row = dst, column = src), in the order given inside a row (stable)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(dst, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    va = np.ones(len(src), np.float32) if va is None else np.asarray(va, np.float32)[order]
    return n, rp, src[order].astype(np.int32), va


def symmetrised(n, rp, ci, va):
    """The pattern plus its transpose (edges only, values 1)."""
    src, dst = S.edges_of(n, rp, ci, va)
    return csr(n, np.concatenate([src, dst]), np.concatenate([dst, src]))


def path(n=65_536, order="index", seed=5):
    """The path name[0] - name[1] - ... - name[n - 1], every edge stored once (name[i] -> name[i + 1])."""
    name = np.arange(n, dtype=np.int64)
    if order == "reversed":
        name = name[::-1].copy()
    elif order == "random":
        name = np.random.default_rng(seed).permutation(n).astype(np.int64)
    return csr(n, name[:-1], name[1:])


def one_way(n=3001, up=True, seed=9):
    """n vertices joined only by edges c -> r with c > r (up) or c < r: a random tree."""
    rng = np.random.default_rng(seed)
    v = np.arange(1, n, dtype=np.int64)
    other = (rng.random(n - 1) * v).astype(np.int64)      # some vertex below v
    return csr(n, v, other) if up else csr(n, other, v)


def hub(k=70_001, where="largest", out=True):
    """A hub joined to k leaves and nothing else; 7 more vertices stay alone.  out: the edges are hub -> leaf (no entry in
    the hub's row: its out-list is the long one); else leaf -> hub (one row of k entries)."""
    n = k + 8
    h = n - 1 if where == "largest" else 0
    leaves = np.arange(1, k + 1, dtype=np.int64)
    hubs = np.full(k, h, np.int64)
    return csr(n, hubs, leaves) if out else csr(n, leaves, hubs)


CLASS_LENGTHS = (0, 1, SHORT, SHORT + 1, PIECE, PIECE + 1, 2 * PIECE + 1)


def class_limits(out):
    """One tying vertex per length of CLASS_LENGTHS, whose list (in-list; out: out-list) of exactly that length is all
    that joins an otherwise separate set of vertices: block k is [base_k, base_k + L_k] with the tying vertex last."""
    src, dst, base = [], [], 0
    for L in CLASS_LENGTHS:
        t = base + L
        members = np.arange(base, t, dtype=np.int64)
        src.append(np.full(L, t, np.int64) if out else members)
        dst.append(members if out else np.full(L, t, np.int64))
        base = t + 1
    n, rp, ci, va = csr(base, np.concatenate(src), np.concatenate(dst))
    lens = np.bincount(ci, minlength=n) if out else np.diff(rp)
    assert set(CLASS_LENGTHS) <= set(lens.tolist())
    return n, rp, ci, va


def grid(side=128):
    """The side x side grid, both directions of every edge stored."""
    v = np.arange(side * side, dtype=np.int64).reshape(side, side)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return csr(side * side, np.concatenate([a, b]), np.concatenate([b, a]))


def pendants(in_giant_rows, giant=20_000, k=500, seed=11, depth=6):
    """A giant (a ring plus random chords, both directions stored, `giant` vertices) and k pendant vertices of larger
    index, each tied in by ONE edge.  in_giant_rows: that edge is stored only in the giant member's row (the pendants'
    rows are empty, and the entry is the last of the member's row, behind the ring's two: it is seen only through a
    pendant's out-list).  Else it is stored only in the pendant's row, at position `depth`, behind edges from `depth`
    private leaves of the pendant (vertices above all pendants): no sampling round with sample <= depth looks at it, and
    it is seen only through the pendant's in-list."""
    rng = np.random.default_rng(seed)
    g = np.arange(giant, dtype=np.int64)
    ca, cb = rng.integers(0, giant, giant // 2), rng.integers(0, giant, giant // 2)
    a = np.concatenate([g, (g + 1) % giant, ca, cb])
    b = np.concatenate([(g + 1) % giant, g, cb, ca])
    pend = giant + np.arange(k, dtype=np.int64)
    anchor = rng.integers(0, giant, k)
    if in_giant_rows:
        n = giant + k
        src, dst = np.concatenate([a, pend]), np.concatenate([b, anchor])      # pendant -> anchor: row = anchor
        return csr(n, src, dst)
    # each pendant's row: `depth` edges from private leaves of its own (vertices above all pendants), then the anchor
    n = giant + k + k * depth
    leaves = giant + k + np.arange(k * depth, dtype=np.int64)
    src = np.concatenate([a, leaves, anchor])
    dst = np.concatenate([b, np.repeat(pend, depth), pend])
    n, rp, ci, va = csr(n, src, dst)
    assert all(ci[rp[q + 1] - 1] < giant and rp[q + 1] - rp[q] == depth + 1 for q in pend[:5])
    return n, rp, ci, va


def no_giant(singles=10_000, pairs=2_000, seed=13):
    """`singles` vertices alone and `pairs` pairs, shuffled."""
    n = singles + 2 * pairs
    name = np.random.default_rng(seed).permutation(n).astype(np.int64)
    return csr(n, name[singles::2], name[singles + 1::2])


def with_noise(n, rp, ci, va, seed=17):
    """The same pattern with stored zeros and columns -1 / n / n + 7 laid over it between vertices of DIFFERENT
    components: if they counted they would join them."""
    rng = np.random.default_rng(seed)
    src, dst = S.edges_of(n, rp, ci, va)
    m = 4 * n
    zs, zd = rng.integers(0, n, m), rng.integers(0, n, m)
    os_ = rng.choice(np.array([-1, n, n + 7]), m)
    od = rng.integers(0, n, m)
    out = csr(n, np.concatenate([src, zs, os_]), np.concatenate([dst, zd, od]),
              np.concatenate([np.ones(len(src), np.float32), np.zeros(m, np.float32), np.ones(m, np.float32)]))
    return out
