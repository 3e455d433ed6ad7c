"""The references of (min,+) on real data and the seeded inputs that tests/test_minplus_ref.py checks on the CPU
and that GPU tests of (min,+) compare the engine with.  numpy / scipy only; not a test and not a conftest.

1. One launch, order-free.  A row computes  out = min(|dot| + |alpha|, |y| + |beta|)  with
dot = min(FLT_MAX, min over its entries of |x[col]| + |a|), x[col] = FLT_MAX for a column outside [0, cols).  Every product
|x| + |a| is ONE float32 addition, rounded on its own; min over floats that are not NaN is exact, commutative and
associative.  So the row's word does not depend on the order, the grouping or the number of partial minima, as long as
no NaN is read: order_free() below (np.minimum.at over the float32 products, seeded with FLT_MAX) and the sequential
O.kernel must agree bit for bit, and so must every plan of the engine.  This is not true of a NaN (clmin's `a < b` is
false for either order), so a row that reads a NaN has no defined word (rows_reading_nan()).

2. A converged SSSP against float64.  Row r reads column c: an edge c -> r of weight |a| (parallel edges: the smaller one
counts, min is idempotent).  With x0 = y0 = FLT_MAX except 0 at the source and alpha = beta = 0 the iteration is
F_(k+1)[r] = min(F_k[r], min_c fl(F_k[c] + |a_rc|)), fl = round to nearest float32.  By induction F_k[r] is the minimum,
over the paths of at most k edges from the source to r, of the path's length added up left to right from the source
in float32 (its "rounded length"); a launch that changes nothing leaves a fixed point F of that map.  Let D be the exact
distance and u = 2^-24.
  upper:  fl is monotone, so along ANY path p_0 = source, .., p_h = r:  F[p_i] <= fl(F[p_(i-1)] + w_i) <= fl(R_(i-1) + w_i) = R_i
          with R the rounded length of the prefix; on the float64 shortest path (h edges) R_h <= D * (1 + u)^h.
  lower:  F[r] is the rounded length of some path of at most L edges (L = launches run); every addition is at least
          (1 - u) times the exact one, so it is >= (that path's exact length) * (1 - u)^L >= D * (1 - u)^L.
So  D * (1 - u)^k <= F <= D * (1 + u)^k  with k = max(h, L).  D here is the exact distance; the float64 reference D64
(Dijkstra's h additions in float64; the weights are float32 numbers and convert exactly) is within
g = h * e / (1 - h * e), e = 2^-53, of it (Higham, lemma 3.1), so the test holds F to
D64 * (1 - u)^k / (1 + g) <= F <= D64 * (1 + u)^k / (1 - g).  There is no absolute term: a float addition whose result is subnormal is
exact.  A vertex without a path keeps FLT_MAX exactly (FLT_MAX + |a| rounds back to FLT_MAX for |a| < 2^103, and every
weight here is below 2^5).  Nothing in this bound is measured on the code under test.
"""
import numpy as np

import float_ref as F

U = 2.0 ** -24
FLT_MAX = np.float32(3.4028235e38)
F32 = np.float32

# (alpha, beta) of every one-launch comparison: the SSSP app's, ordinary, negative with a subnormal, huge
EPILOGUES = ((0.0, 0.0), (0.25, 1.5), (-3.5, -2.0 ** -130), (2.0 ** 100, 0.0))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_of_entries(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))


# ------------------------------------------------------------------ 1. one launch, order-free
def order_free(rp, ci, va, x, y, alpha, beta, cols, keep_sign_of_values=False):
    """One (min,+) launch in numpy float32 without any order: see the module docstring.  `keep_sign_of_values` is the
    mutant that drops fabsf() from the matrix value inside the product (clmin still takes the magnitude)."""
    rows = len(rp) - 1
    ci = np.asarray(ci, np.int64)
    va = np.ascontiguousarray(va, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    inside = (ci >= 0) & (ci < cols)
    xv = np.full(len(ci), FLT_MAX, np.float32)
    xv[inside] = x[ci[inside]]
    with np.errstate(over="ignore", invalid="ignore"):
        prod = np.abs(xv) + (va if keep_sign_of_values else np.abs(va))      # float32 + float32: one rounding
        prod = np.abs(prod)
        dot = np.full(rows, FLT_MAX, np.float32)
        np.minimum.at(dot, rows_of_entries(rp), prod)
        a = np.abs(dot) + np.abs(F32(alpha))
        b = np.abs(np.ascontiguousarray(y, np.float32)) + np.abs(F32(beta))
        out = np.minimum(a, b)
    assert out.dtype == np.float32
    return out


def rows_reading_nan(rp, ci, va, x, y, cols):
    """The rows whose word is undefined: a NaN value, a NaN x[col] of an in-range entry, or a NaN y.  From the inputs alone."""
    ci = np.asarray(ci, np.int64)
    inside = (ci >= 0) & (ci < cols)
    bad = np.isnan(np.asarray(va, np.float32))
    bad[inside] |= np.isnan(np.asarray(x, np.float32))[ci[inside]]
    out = np.isnan(np.asarray(y, np.float32)).copy()
    out[rows_of_entries(rp)[bad]] = True
    return out


def nan_case(c, seed=94):
    """The ragged input set `c` with one NaN x column, ten NaN weights and three NaN y.  The long rows (>= 4095 entries)
    read nearly every column, so their entries that pointed at the NaN column are moved to its neighbour: they stay
    clean by construction.  The exempt set comes from the inputs alone, stays under 1 % of the rows and holds no long
    row.  -> (rp, ci, va, x, y, exempt rows)"""
    rng = np.random.default_rng(seed)
    rp, ci, va, x, y = c["rp"], c["ci"].copy(), c["va"].copy(), c["x"].copy(), c["y"].copy()
    long_rows = np.nonzero(np.diff(rp) >= 4095)[0]
    col = 777
    is_long = np.isin(rows_of_entries(rp), long_rows)
    ci[is_long & (ci == col)] = col + 1
    x[col] = np.nan
    # NaN weights in short and medium rows only: rows that share a fold, a column tile or a stream block with them
    cand = np.nonzero(~is_long & (ci >= 0) & (ci < c["cols"]))[0]
    va[rng.choice(cand, 10, replace=False)] = np.where(rng.random(10) < 0.5, np.float32(np.nan), -np.float32(np.nan))
    y[rng.choice(np.setdiff1d(np.arange(c["rows"]), long_rows), 3, replace=False)] = np.nan
    exempt = rows_reading_nan(rp, ci, va, x, y, c["cols"])
    assert len(long_rows) >= 8 and 20 < exempt.sum() < 0.01 * c["rows"] and not exempt[long_rows].any()
    return rp, ci, va, x, y, exempt


# ------------------------------------------------------------------ 2. converged SSSP against float64
def float64_sssp(rp, ci, va, source):
    """-> (D, hops): scipy's Dijkstra in float64 on the edges col -> row of weight |a| (parallel edges reduced by min,
    columns outside [0, n) dropped), and the number of edges of every vertex' path in its shortest-path tree
    (-1: unreached, D = inf)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    n = len(rp) - 1
    ci = np.asarray(ci, np.int64)
    inside = (ci >= 0) & (ci < n)
    src, dst = ci[inside], rows_of_entries(rp)[inside]
    w = np.abs(np.asarray(va, np.float64))[inside]
    assert (w > 0).all(), "csgraph drops explicit zeros: keep the weights positive"
    order = np.lexsort((w, dst, src))                 # the lightest of a bundle of parallel edges first
    src, dst, w = src[order], dst[order], w[order]
    first = np.ones(len(src), bool)
    first[1:] = (src[1:] != src[:-1]) | (dst[1:] != dst[:-1])
    g = csr_matrix((w[first], (src[first], dst[first])), shape=(n, n))
    D, pred = dijkstra(g, directed=True, indices=int(source), return_predecessors=True)
    hops = np.where(np.isfinite(D), 0, -1).astype(np.int64)
    todo = np.nonzero(pred >= 0)[0]
    at = pred[todo].astype(np.int64)
    while len(todo):                                  # walk every vertex up its tree path, one edge per round
        hops[todo] += 1
        alive = pred[at] >= 0
        todo, at = todo[alive], pred[at[alive]].astype(np.int64)
    return D, hops


def path_bound(D, hops, launches):
    """-> (lo, hi) per vertex, float64; for an unreached vertex both are FLT_MAX (it must be FLT_MAX exactly)."""
    reached = np.isfinite(D)
    k = np.maximum(hops, launches).astype(np.float64)
    g = np.maximum(hops, 0) * 2.0 ** -53 / (1.0 - np.maximum(hops, 0) * 2.0 ** -53)     # the float64 reference's own error
    lo = np.where(reached, D * (1.0 - U) ** k / (1.0 + g), float(FLT_MAX))
    hi = np.where(reached, D * (1.0 + U) ** k / (1.0 - g), float(FLT_MAX))
    return lo, hi


def path_ratios(got, D, hops, launches):
    """(got - D) / (allowed deviation on that side) per vertex: within the bound iff |ratio| <= 1; inf for an unreached
    vertex that is not FLT_MAX exactly or for a reached one that is not finite."""
    got64 = np.asarray(got, np.float64)
    lo, hi = path_bound(D, hops, launches)
    reached = np.isfinite(D)
    r = np.zeros(len(D))
    with np.errstate(divide="ignore", invalid="ignore"):
        up, down = got64 - D, D - got64
        r[reached] = np.where(up >= 0, up / (hi - D), down / (D - lo))[reached]
    r[reached & (D == 0)] = np.where(got64[reached & (D == 0)] == 0, 0.0, np.inf)     # the source
    r[~reached] = np.where(bits(got)[~reached] == bits(FLT_MAX)[0], 0.0, np.inf)
    return np.where(np.isnan(r), np.inf, r)


def assert_within_path_bound(got, D, hops, launches, what=""):
    r = path_ratios(got, D, hops, launches)
    worst = int(np.argmax(r))
    print(f"[minplus bound] {what}: worst err/bound {r[worst]:.3f} at vertex {worst} ({int(hops[worst])} hops, {launches} launches, "
          f"{int(np.isfinite(D).sum())} of {len(D)} reached)")
    bad = np.nonzero(r > 1.0)[0]
    if len(bad):
        lines = [f"vertex {i}: got {float(got[i])!r}, float64 {D[i]!r}, {int(hops[i])} hops, err/bound {r[i]:.3f}" for i in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} vertices outside the float64 path bound\n" + "\n".join(lines))
    return float(r[worst])


# ------------------------------------------------------------------ 3. seeded inputs
def with_unreached(rng, v, share=0.3):
    """`v` with `share` of its entries replaced by +-FLT_MAX (unreached vertices; the sign must not matter)."""
    v = v.copy()
    hit = rng.random(len(v)) < share
    v[hit] = np.where(rng.random(int(hit.sum())) < 0.5, FLT_MAX, -FLT_MAX)
    return v


def one_launch_case(c, seed):
    """A float_ref input set (real, mixed-sign weights, x, y and further columns) with a share of +-FLT_MAX in every
    x and y, each vector with a pattern of its own."""
    rng = np.random.default_rng(seed)
    c = dict(c)
    c["x"], c["y"] = with_unreached(rng, c["x"]), with_unreached(rng, c["y"])
    c["xs"] = [with_unreached(rng, v) for v in c["xs"]]
    c["ys"] = [with_unreached(rng, v) for v in c["ys"]]
    return c


def generators(clustered_matrix):
    """name -> f(width) of the six one-launch input sets (clustered_matrix: the function of tests/test_parity_gpu.py)."""
    return {
        "ragged": lambda width=0: one_launch_case(F.gen_ragged(width), 201),
        "clustered": lambda width=0: one_launch_case(F.gen_clustered(clustered_matrix, width), 202),
        "wide": lambda width=0: one_launch_case(F.gen_wide(width), 203),
        "few16": lambda width=0: one_launch_case(F.gen_few_values(16, width), 204),
        "few255": lambda width=0: one_launch_case(F.gen_few_values(255, width), 205),
        "few4000": lambda width=0: one_launch_case(F.gen_few_values(4000, width), 206),
    }


def real_weights(rng, nnz):
    """exp(U(-6, 3)), a random third of them negated: 0.0025 .. 20, nine binades, no two launches alike in their low bits."""
    w = np.exp(rng.uniform(-6.0, 3.0, nnz))
    w[rng.random(nnz) < 1.0 / 3.0] *= -1.0
    return w.astype(np.float32)


def weighted_rmat(scale=15, seed=61):
    from sparseharness_amd import hostlib as H
    rp, ci, _ = H.rmat(scale, seed=seed)
    return rp, ci, real_weights(np.random.default_rng(seed + 1), len(ci)), 1 << scale


def weighted_grid(h=120, w=250, seed=63):
    """4-neighbour grid, vertex (i, j) = i * w + j: hundreds of launches with a thin wavefront each."""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src, dst = [], []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        src += [a.ravel(), b.ravel()]
        dst += [b.ravel(), a.ravel()]
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=h * w))]).astype(np.int32)
    return rp, dst.astype(np.int32), real_weights(np.random.default_rng(seed), len(dst)), h * w


GRAPHS = {"rmat15": weighted_rmat, "grid": weighted_grid}
_graphs = {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = GRAPHS[name]()
    return _graphs[name]


def sources(name):
    """Vertex 0 (the apps' source) and two more; on the R-MAT, vertices that at least eight rows read (an isolated source
    would reach nobody)."""
    rp, ci, _, n = graph(name)
    if name == "grid":
        return (0, n // 2 + 17, n - 1)
    read_by = np.bincount(ci[(ci >= 0) & (ci < n)], minlength=n)
    cand = np.random.default_rng(62).permutation(np.arange(1, n))
    return (0,) + tuple(int(v) for v in cand[read_by[cand] >= 8][:2])


def start_vector(n, source):
    v = np.full(n, FLT_MAX, np.float32)
    v[source] = 0.0
    return v


def launch_changes(kernel, rp, ci, va, x0, launches):
    """The size of every vertex improvement |x_k - x_(k+1)| > 0 of the first `launches` launches of the SSSP iteration
    run with `kernel` (the ORACLE's one-launch function), unreached -> reached steps left out.  For picking a delta that
    many improvements fall below."""
    out, x = [], x0
    for _ in range(launches):
        nxt = kernel(rp, ci, va, x, x)
        moved = (bits(nxt) != bits(x)) & (np.abs(x) < FLT_MAX)
        out.append(np.abs(x[moved].astype(np.float64) - nxt[moved]))
        x = nxt
    return np.concatenate(out) if out else np.zeros(0)
