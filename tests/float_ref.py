"""The float64 reference of (+,x) and the bound a float32 result is held to, plus the seeded inputs that
tests/test_float_bound.py (CPU) and tests/test_float_gpu.py (GPU) share.  numpy float64 only; not a conftest.

The bound.  A row computes  out = (dot * alpha) + (y * beta)  with  dot = sum of n products va * x[col]  in float32.
With u = 2^-24 (round to nearest) and gamma(k) = k*u / (1 - k*u)  (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 3.1 / lemma 3.1), ANY order of the n - 1 additions -- sequential, tree, segments combined
afterwards -- puts at most n - 1 roundings on a product's path to the sum; the product itself is one more, or none
when a multiply and its add are contracted into one rounding.  dot * alpha, y * beta and the final add put at most two
more on either term.  That is n + 2 factors (1 + d), |d| <= u, at the most; one is held in reserve for an explicit
"+ 0" seed of a partial sum:

    |got - exact| <= gamma(n + 3) * (|alpha| * sum|va * x| + |y * beta|) + (n + 3) * 2^-149

The last term covers underflow: each of the at most n + 3 operations that rounds into the subnormal range adds an
absolute error of at most half a subnormal spacing, 2^-150 (additions are exact there; products are not), and a later
factor (1 + d) or |alpha| scales it -- twice as much is allowed for that, which assumes |alpha| <= 2 for the products
that underflow (true of every case here: the tiny-alpha case scales errors DOWN).  Nothing here is measured on the code under test.
"""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def exact_rows(rp, ci, va, x, cols):
    """-> (dot, mag, n) per row: the float64 sum of va * x[ci] over the entries whose column lies in [0, cols), the sum
    of |va * x[ci]|, and the number of such entries.  (A float64 sum of n terms is itself within n * 2^-53 * mag of the
    true sum: 2^-29 of the float32 bound, ignored.)"""
    rp = np.asarray(rp, np.int64)
    rows = len(rp) - 1
    ci = np.asarray(ci, np.int64)
    inside = (ci >= 0) & (ci < cols)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))[inside]
    prod = np.asarray(va, np.float64)[inside] * np.asarray(x, np.float64)[ci[inside]]
    dot = np.bincount(row_of, weights=prod, minlength=rows)
    mag = np.bincount(row_of, weights=np.abs(prod), minlength=rows)
    n = np.bincount(row_of, minlength=rows)
    return dot, mag, n


def f32(v):
    """The float32 the engine receives for a scalar, as a float64."""
    return float(np.float32(v))


def bound(n, mag, alpha, y, beta):
    n = np.asarray(n, np.float64)
    yb = 0.0 if y is None else np.abs(np.asarray(y, np.float64) * f32(beta))
    return gamma(n + 3) * (abs(f32(alpha)) * np.asarray(mag, np.float64) + yb) + (n + 3) * 2.0 ** -149


def exact_out(dot, alpha, y, beta):
    return dot * f32(alpha) + (0.0 if y is None else np.asarray(y, np.float64) * f32(beta))


def ratios(got, dot, mag, n, alpha, y, beta):
    """err / bound per row (inf where `got` is not finite)."""
    err = np.abs(np.asarray(got, np.float64) - exact_out(dot, alpha, y, beta))
    r = err / bound(n, mag, alpha, y, beta)
    return np.where(np.isfinite(r), r, np.inf)


def assert_within(got, dot, mag, n, alpha, y, beta, what=""):
    """Every row of `got` within bound() of the float64 result; prints and returns the worst err / bound."""
    r = ratios(got, dot, mag, n, alpha, y, beta)
    worst = int(np.argmax(r)) if len(r) else 0
    print(f"[float bound] {what}: worst err/bound {r[worst] if len(r) else 0.0:.3f} at row {worst} ({int(n[worst]) if len(r) else 0} entries)")
    bad = np.nonzero(r > 1.0)[0]
    if len(bad):
        want = exact_out(dot, alpha, y, beta)
        lines = [f"row {i}: {int(n[i])} entries, got {float(got[i])!r}, exact {want[i]!r}, err/bound {r[i]:.3f}" for i in bad[:8]]
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} rows outside the float32 bound\n" + "\n".join(lines))
    return float(r[worst]) if len(r) else 0.0


# ------------------------------------------------------------------ narrower floats (what a lossy layout would carry)
def to_bf16_trunc(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def to_fp16_round(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, np.float32).astype(np.float16).astype(np.float32)


def to_mant10_trunc(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)


NARROWINGS = {"bf16": to_bf16_trunc, "fp16": to_fp16_round, "mant10": to_mant10_trunc}


# ------------------------------------------------------------------ seeded inputs
def wide_range(rng, n):
    """normal * e^U(-8, 8): mixed signs, six and a half decades of magnitude."""
    return (rng.standard_normal(n) * np.exp(rng.uniform(-8.0, 8.0, n))).astype(np.float32)


RAGGED_LENGTHS = (0, 1, 16, 17, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 70001)
RAGGED_ROWS, RAGGED_COLS = 6000, 5000


def ragged_pattern(seed=5):
    """6000 x 5000: rows of 0..64 entries, a fifth of them empty, one row of each length in RAGGED_LENGTHS (around the
    one-team limit, a stream block, a long-row segment and several segments), 2 % of the columns outside [0, cols) on
    either side, and one hub column that 5 % of the entries point at.  -> (rp, ci, rng)"""
    rng = np.random.default_rng(seed)
    rows, cols = RAGGED_ROWS, RAGGED_COLS
    deg = rng.integers(0, 65, rows).astype(np.int64)
    deg[rng.random(rows) < 0.2] = 0
    deg[100 + 397 * np.arange(len(RAGGED_LENGTHS))] = RAGGED_LENGTHS
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    ci[rng.random(nnz) < 0.05] = 1234
    stray = rng.random(nnz) < 0.02
    k = int(stray.sum())
    ci[stray] = np.where(rng.random(k) < 0.5, -1 - rng.integers(0, 5, k), cols + rng.integers(0, 1000, k)).astype(np.int32)
    return rp, ci, rng


def case(rows, cols, rp, ci, va, rng, width=0):
    """One input set: the matrix, x and y (and `width` further x / y columns for the multi-vector entry points)."""
    xs = [wide_range(rng, cols) for _ in range(1 + width)]
    ys = [wide_range(rng, rows) for _ in range(1 + width)]
    return dict(rows=rows, cols=cols, rp=rp, ci=ci, va=va, x=xs[0], y=ys[0], xs=xs[1:], ys=ys[1:])


def gen_ragged(width=0):
    rp, ci, rng = ragged_pattern()
    return case(RAGGED_ROWS, RAGGED_COLS, rp, ci, wide_range(rng, int(rp[-1])), rng, width)


def gen_clustered(clustered_matrix, width=0):
    """clustered_matrix() of tests/test_parity_gpu.py (passed in: this module imports no test) with real weights."""
    rp, ci, _, n = clustered_matrix(seed=12)
    rng = np.random.default_rng(14)
    return case(n, n, rp, ci, wide_range(rng, int(rp[-1])), rng, width)


def gen_wide(width=0):
    """20 000 x 2 500 000: x spans ~77 column tiles of the tiled plan; a few hundred-entry rows and two heavy ones."""
    rng = np.random.default_rng(15)
    rows, cols = 20_000, 2_500_000
    deg = rng.poisson(10, rows).astype(np.int64)
    deg[rng.integers(0, rows, 200)] = rng.integers(100, 700, 200)
    deg[[11, rows - 5]] = (9000, 30_000)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    return case(rows, cols, rp, ci, wide_range(rng, nnz), rng, width)


def gen_few_values(distinct, width=0):
    """`distinct` different real values, negative ones included, none zero, all finite: the coded layouts of the tiled plan."""
    rng = np.random.default_rng(1000 + distinct)
    rows, cols = 30_000, 100_000
    deg = rng.poisson(9, rows).astype(np.int64)
    deg[rng.integers(0, rows, 5)] = 4000
    deg[rng.integers(0, rows, 300)] = rng.integers(30, 300, 300)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    pool = np.unique(wide_range(rng, 2 * distinct + 64))
    pool = pool[pool != 0][:: max(1, len(pool) // distinct)][:distinct]
    assert len(pool) == distinct and (pool < 0).any() and (pool > 0).any()
    va = pool[rng.integers(0, distinct, nnz)]
    va[:distinct] = pool
    return case(rows, cols, rp, ci, va.astype(np.float32), rng, width)


EPILOGUES = ((1.0, 0.0, False), (-1.7, 0.3, True), (2.0 ** -20, 2.0 ** 20, True))   # (alpha, beta, with y)
