"""Reference for sh_tri (tests/test_tri_ref.py pins it against closed forms and the host gold, tests/test_tri_gpu.py
compares the engine with it): counts() gives the triangles through every vertex, the degrees and the number of edges
of the simple undirected graph under a CSR pattern -- densely as diag(A^3) / 2 up to 2048 vertices, with Python sets
above -- and the makers of the patterns the GPU tests run on.  No line here is shared with the product."""
import numpy as np

from wcc_ref import csr

# the list-length classes of the kernels (tri.hip.h: TRI_SHORT, TRI_WAVE, TRI_CHUNK); tests/test_tri_ref.py reads the
# header and asserts that the two agree
SHORT, WAVE, CHUNK = 8, 512, 2048
CLASS_LENGTHS = (SHORT, SHORT + 1, WAVE, WAVE + 1, CHUNK, CHUNK + 1)
DENSE_LIMIT = 2048


def pairs_of(n, rp, ci, va):
    """The edges {u, v} of the simple undirected graph as two arrays u < v, each edge once: entry (r, c) counts when
    0 <= c < n, c != r and its 32 value bits are not all zero."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    bits = np.ascontiguousarray(va).view(np.uint32)
    keep = (bits != 0) & (ci >= 0) & (ci < n) & (ci != row)
    lo, hi = np.minimum(row[keep], ci[keep]), np.maximum(row[keep], ci[keep])
    code = np.unique(lo * max(n, 1) + hi)
    return code // max(n, 1), code % max(n, 1)


def counts(n, rp, ci, va):
    """-> (tri, deg, M): tri[v] (uint64) the triangles through v, deg[v] (int32) its degree, M the number of edges."""
    u, v = pairs_of(n, rp, ci, va)
    deg = (np.bincount(u, minlength=n) + np.bincount(v, minlength=n)).astype(np.int32)[:n]
    if n <= DENSE_LIMIT:
        # closed walks of length 3 from v: each triangle through v is walked in two directions.  The product runs in
        # float64 (numpy has no fast integer matmul) and is exact: no entry of A @ A exceeds 2048, no sum 2^22; the
        # counts are int64 from there on
        A = np.zeros((n, n), np.float64)
        A[u, v] = 1.0
        A[v, u] = 1.0
        walks = np.einsum("ij,ji->i", A @ A, A)
        tri = np.rint(walks).astype(np.int64) // 2
        return tri.astype(np.uint64), deg, len(u)
    nb = [set() for _ in range(n)]
    for a, b in zip(u.tolist(), v.tolist()):
        nb[a].add(b)
        nb[b].add(a)
    twice = np.zeros(n, np.int64)   # every triangle through x is met at two of x's edges
    for a, b in zip(u.tolist(), v.tolist()):
        k = len(nb[a] & nb[b])
        twice[a] += k
        twice[b] += k
    return (twice // 2).astype(np.uint64), deg, len(u)


def from_pairs(n, a, b, both=True):
    """CSR arrays of the edges a[i] - b[i]: stored in both rows, or (both = False) in row b[i] only."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return csr(n, np.concatenate([a, b]), np.concatenate([b, a])) if both else csr(n, a, b)


def complete(n):
    a, b = np.triu_indices(n, 1)
    return from_pairs(n, a, b)


def friendship(k, hub="first"):
    """A hub tied to 2k leaves, leaf 2i tied to leaf 2i + 1: k triangles, tri[hub] = k and 1 for every leaf.  hub: the
    vertex of index 0 ("first") or n - 1 ("last")."""
    n = 2 * k + 1
    h = 0 if hub == "first" else n - 1
    leaves = np.arange(2 * k, dtype=np.int64) + (1 if hub == "first" else 0)
    return from_pairs(n, np.concatenate([np.full(2 * k, h, np.int64), leaves[0::2]]), np.concatenate([leaves, leaves[1::2]]))


def bipartite(a, b):
    """K_{a,b}: no triangle, a * b * (a + b - 2) / 2 wedges."""
    x, y = np.meshgrid(np.arange(a, dtype=np.int64), a + np.arange(b, dtype=np.int64), indexing="ij")
    return from_pairs(a + b, x.ravel(), y.ravel())


def triangulated_grid(side):
    """The side x side grid with one diagonal per cell: 2 * (side - 1)^2 triangles."""
    v = np.arange(side * side, dtype=np.int64).reshape(side, side)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel(), v[:-1, :-1].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel(), v[1:, 1:].ravel()])
    return from_pairs(side * side, a, b)


def pattern(n=700, m=6000, seed=3):
    """A random simple pattern, stored in both rows (the base of the storage forms below)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    return from_pairs(n, a[a != b], b[a != b])


def upper_only(n, rp, ci, va):
    u, v = pairs_of(n, rp, ci, va)
    return csr(n, v, u)      # row u stores column v > u


def lower_only(n, rp, ci, va):
    u, v = pairs_of(n, rp, ci, va)
    return csr(n, u, v)      # row v stores column u < v


def one_way_triangles(t=400, seed=7):
    """t triangles over 2 * t vertices, every one stored as a -> b, b -> c, c -> a only (no entry has its mirror, unless
    another triangle brings it)."""
    rng = np.random.default_rng(seed)
    n = 2 * t
    tr = np.array([rng.choice(n, 3, replace=False) for _ in range(t)], np.int64)
    src = np.concatenate([tr[:, 0], tr[:, 1], tr[:, 2]])
    dst = np.concatenate([tr[:, 1], tr[:, 2], tr[:, 0]])
    return csr(n, src, dst)


def with_noise(n, rp, ci, va, seed=17):
    """The same graph with stored zeros and columns -1 / n / n + 7 laid over it (if they counted they would add edges and
    close triangles), plus self-loops and every entry that counts stored a second time."""
    rng = np.random.default_rng(seed)
    rp64 = np.asarray(rp, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp64))
    col = np.asarray(ci, np.int64)
    m = 4 * n
    zs, zd = rng.integers(0, n, m), rng.integers(0, n, m)
    os_, od = rng.choice(np.array([-1, n, n + 7]), m), rng.integers(0, n, m)
    loops = rng.integers(0, n, n // 2 + 1)
    src = np.concatenate([col, col, zs, os_, loops])
    dst = np.concatenate([row, row, zd, od, loops])
    val = np.concatenate([np.asarray(va, np.float32), np.asarray(va, np.float32), np.zeros(m, np.float32),
                          np.ones(m, np.float32), np.ones(len(loops), np.float32)])
    return csr(n, src, dst, val)


def noise_as_edges(n, rp, ci, va):
    """with_noise's pattern with every stored zero set to one: what the graph would be if zeros counted."""
    return n, rp, ci, np.ones(len(ci), np.float32)


def class_limits():
    """One vertex per forward-list length of CLASS_LENGTHS under order = 0: a fan per length L, its hub the smallest
    index of the fan, tied to L rim vertices that form a path (L - 1 triangles through the hub).  Under order = 1 the
    rims (degree <= 3) point at the hubs and every list is short; a forward list of L entries there needs L neighbours
    of degree >= L, so K_10 and K_514 follow for the limits at 8 and 512, and the chunk boundary at 2048 is left to
    K_2400 (tests/test_tri_gpu.py)."""
    a, b, base = [], [], 0
    for L in CLASS_LENGTHS:
        rim = base + 1 + np.arange(L, dtype=np.int64)
        a += [np.full(L, base, np.int64), rim[:-1]]
        b += [rim, rim[1:]]
        base += L + 1
    for k in (SHORT + 2, WAVE + 2):
        x, y = np.triu_indices(k, 1)
        a.append(base + x)
        b.append(base + y)
        base += k
    n, rp, ci, va = from_pairs(base, np.concatenate(a), np.concatenate(b))
    u, v = pairs_of(n, rp, ci, va)
    assert set(CLASS_LENGTHS) <= set(np.bincount(u, minlength=n).tolist())   # forward lengths under order = 0
    return n, rp, ci, va
