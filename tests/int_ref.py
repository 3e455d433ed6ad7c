"""The reference of the two integer semirings, (or,and) and (max,min) on int32, written from their definition
(sparseharness_amd/csrc/semiring.hip.h), and the seeded inputs that tests/test_int_ref.py (CPU), tests/test_plan_cpu.py
(host emulator) and tests/test_int_gpu.py (GPU) share.  Plain numpy in int64 and Python ints; nothing here comes from the
engine, and from the oracle only the semiring ids.  Not a test and not a conftest.

Every element is a 32-bit WORD.  Both semirings are exact and order-free on words -- min, max, != 0 have no rounding and
max / OR are associative and commutative -- so every comparison made with this module is == on uint32 views; there is no
tolerance anywhere.

  (max,min)  dot = max(INT_MIN, max over the row's entries of min(x[col], a)),  x[col] = INT_MIN outside [0, cols)
             out = max(min(dot, alpha), min(y, beta));  y is not read when beta == INT_MIN (min(y, INT_MIN) == INT_MIN)
  (or,and)   dot = OR over the row's entries of (x[col] != 0 && a != 0),        x[col] = 0 outside [0, cols)
             out = (dot && alpha != 0) || (y != 0 && beta != 0), as 0 / 1;      y is not read when beta == 0

The word pool SPECIAL holds the words at which a kernel that leaves the integer view goes wrong: a compare or min / max
in the float view (-0.0 == +0.0, NaN unordered, negative order reversed), a move that quiets a signalling NaN or
flushes a subnormal, a trip through float (2^24 + 1), a 16-bit truncation, a compare by subtraction (INT_MAX against
-1), a padding word of 0 in a row whose result is negative.  tests/test_int_ref.py shows on these inputs that each of
those mistakes, made in this reference, changes at least 1 % of the non-empty rows.
"""
import numpy as np

import float_ref as F
import graph_patterns as P

OR_AND, MAX_MIN = 2, 3     # oracle.OR_AND_I32, oracle.MAX_MIN_I32 (pinned against the oracle in tests/test_int_ref.py)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def i32(w):
    """A word given as 0 .. 2^32 - 1 or as a signed int -> the signed Python int the engine's scalars are passed as."""
    w = int(w) & 0xFFFFFFFF
    return w - (1 << 32) if w >= 1 << 31 else w


SPECIAL = np.array([
    0, 1, 0xFFFFFFFF, 2, 0x80000000, 0x80000001, 0x7FFFFFFF, 0x7FFFFFFE,     # 0, 1, -1, 2, INT_MIN (-0.0), INT_MIN + 1, INT_MAX, INT_MAX - 1
    0x7F800000, 0xFF800000,                                                  # +-Inf
    0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,                          # quiet and signalling NaNs
    0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,                          # subnormals
    0x7F7FFFFF,                                                              # FLT_MAX, the (min,+) identity
    0x00010000, 0xFFFF0000, 0x0000FFFF,                                      # the halves of a word
    0x01000000, 0x01000001, 0xFF000000, 0xFEFFFFFF,                          # 2^24, 2^24 + 1, -(2^24), -(2^24 + 1)
], np.uint32).view(np.int32)
NAN_WORD = i32(0x7FC00000)
# Words that are not zero but that a float view (-0.0) or a view of the low 16 bits takes for zero
LOOK_LIKE_ZERO = np.array([0x80000000, 0x80000000, 0x00010000, 0xFFFF0000], np.uint32).view(np.int32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words(rng, n, special_share=1.0 / 3.0):
    """n int32 words: `special_share` of them drawn from SPECIAL, the rest uniform over all 2^32 words."""
    out = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    hit = rng.random(n) < special_share
    out[hit] = SPECIAL[rng.integers(0, len(SPECIAL), int(hit.sum()))]
    return out


def negative_words(rng, n, special_share=1.0 / 3.0):
    """words() with the sign bit set: every word < 0 (INT_MIN, -1, the negative NaNs and subnormals among them)."""
    return (bits(words(rng, n, special_share)) | np.uint32(0x80000000)).view(np.int32)


def truth_words(rng, n):
    """The (or,and) inputs: a third exactly 0, a third of LOOK_LIKE_ZERO (half of those INT_MIN), a third words().  Only
    the class of a word matters to (or,and); with the plain third of zeros alone a row's truth hangs on ONE word that
    looks like zero in under 0.2 % of the rows of `ragged` (measured on this reference), below what test_int_ref.py asks."""
    out = words(rng, n)
    kind = rng.integers(0, 3, n)
    out[kind == 0] = 0
    out[kind == 1] = LOOK_LIKE_ZERO[rng.integers(0, len(LOOK_LIKE_ZERO), int((kind == 1).sum()))]
    return out


# ------------------------------------------------------------------ one launch, from the definition
def rows_of_entries(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))


def reduce_rows(op, rp, prod, identity):
    """op.reduce over every row's products (int64), `identity` for a row without entries."""
    rp = np.asarray(rp, np.int64)
    out = np.full(len(rp) - 1, identity, np.int64)
    full = np.diff(rp) > 0
    if full.any():   # (the starts of the non-empty rows ascend strictly and each run ends where the next one starts)
        out[full] = op.reduceat(prod, rp[:-1][full])
    return out


def gather(x, ci, cols, identity):
    """x[col] per entry as int64, `identity` for a column outside [0, cols)."""
    ci = np.asarray(ci, np.int64)
    inside = (ci >= 0) & (ci < cols)
    xv = np.full(len(ci), identity, np.int64)
    xv[inside] = np.asarray(x).astype(np.int64)[ci[inside]]
    return xv


def reads_y(sr, beta):
    return i32(beta) != (0 if sr == OR_AND else INT_MIN)


def kernel(sr, rp, ci, va, x, y, alpha, beta, cols):
    """One launch -> int32[rows].  y may be None when reads_y(sr, beta) is false."""
    alpha, beta = i32(alpha), i32(beta)
    a = np.asarray(va).astype(np.int64)
    yv = np.asarray(y).astype(np.int64) if reads_y(sr, beta) else None
    if sr == MAX_MIN:
        dot = np.maximum(reduce_rows(np.maximum, rp, np.minimum(gather(x, ci, cols, INT_MIN), a), INT_MIN), INT_MIN)
        m1 = np.minimum(dot, alpha)
        m2 = np.minimum(yv, beta) if yv is not None else INT_MIN
        return np.maximum(m1, m2).astype(np.int32)
    assert sr == OR_AND
    dot = reduce_rows(np.logical_or, rp, (gather(x, ci, cols, 0) != 0) & (a != 0), False) != 0
    r1 = dot & (alpha != 0)
    r2 = (yv != 0) & (beta != 0) if yv is not None else False
    return (r1 | r2).astype(np.int32)


def iterate(sr, rp, ci, va, x0, y0, alpha, beta, max_iters):
    """The iterative apps' loop on a square matrix: launch, compare the input with the output word for word, go on from
    the output with y = the new input.  -> (vector, launches including the confirming one, converged)"""
    n = len(rp) - 1
    x, y = np.ascontiguousarray(x0, np.int32), np.ascontiguousarray(y0, np.int32)
    it, same = 0, False
    while True:
        out = kernel(sr, rp, ci, va, x, y, alpha, beta, n)
        same = bool(np.array_equal(bits(x), bits(out)))
        x = y = out
        it += 1
        if same or it >= max_iters:
            return x, it, same


# ------------------------------------------------------------------ seeded inputs
# (alpha, beta, with y) of every one-launch comparison
EPILOGUES = {
    MAX_MIN: ((INT_MAX, INT_MIN, False), (INT_MAX, INT_MAX, True), (-5, INT_MIN + 1, True), (INT_MIN, 7, True),
              (i32(0x7FC00000), i32(0x80000001), True)),
    OR_AND: ((1, 0, False), (1, 1, True), (INT_MIN, INT_MIN, True), (0, i32(0x00010000), True), (i32(0x7F800001), 0, False)),
}
WIDTH = 32   # further x / y columns of an input set (the multi-vector entry points)


def near_ties(rng, ci, va, x, cols, share=0.1):
    """`share` of the in-range values replaced by x[col] - 1 or x[col] + 1 (wrapping): two words that one rounding to
    float32 makes equal wherever |x| >= 2^25, and that a compare has to tell apart all the same."""
    inside = np.nonzero((ci >= 0) & (ci < cols))[0]
    pick = inside[rng.random(len(inside)) < share]
    va = va.copy()
    step = np.where(rng.random(len(pick)) < 0.5, -1, 1).astype(np.int64)
    va[pick] = (x[ci[pick]].astype(np.int64) + step).astype(np.uint32).view(np.int32)   # (wraps at the ends of the range)
    return va


def case(sr, rows, cols, rp, ci, rng, pool=None, width=0):
    """One input set of semiring `sr` on the pattern (rp, ci): values, x, y and `width` further x / y columns.  (max,min):
    words() everywhere and, where the values are not a fixed pool, near_ties().  (or,and): truth_words() for x and the
    values, words() for y.  `pool`: the distinct words the values are drawn from (a few-values input)."""
    nnz = int(rp[-1])
    draw = truth_words if sr == OR_AND else words
    xs = [draw(rng, cols) for _ in range(1 + width)]
    ys = [words(rng, rows) for _ in range(1 + width)]
    if pool is not None:
        va = pool[rng.integers(0, len(pool), nnz)]
        va[:len(pool)] = pool                      # every word occurs
        if sr == OR_AND:
            va[rng.random(nnz) < 1.0 / 3.0] = 0
            va[:len(pool)] = pool
    elif sr == OR_AND:
        va = truth_words(rng, nnz)
    else:
        va = near_ties(rng, ci, words(rng, nnz), xs[0], cols)
    return dict(sr=sr, rows=rows, cols=cols, rp=rp, ci=ci, va=np.ascontiguousarray(va, np.int32), x=xs[0], y=ys[0], xs=xs[1:], ys=ys[1:])


def gen_ragged(sr, width=0):
    rp, ci, rng = F.ragged_pattern()
    return case(sr, F.RAGGED_ROWS, F.RAGGED_COLS, rp, ci, rng, width=width)


def gen_clustered(sr, clustered_matrix, width=0):
    """clustered_matrix() of tests/test_parity_gpu.py (passed in: this module imports no test)."""
    rp, ci, _, n = clustered_matrix(seed=12)
    return case(sr, n, n, rp, ci, np.random.default_rng(14 + sr), width=width)


def gen_wide(sr, width=0):
    c = F.gen_wide()
    return case(sr, c["rows"], c["cols"], c["rp"], c["ci"], np.random.default_rng(15 + sr), width=width)


def value_pool(rng, distinct):
    """`distinct` different words of words(), always with 0, INT_MIN and one NaN pattern among them."""
    must = np.array([0, INT_MIN, NAN_WORD], np.int64)
    drawn = words(rng, 2 * distinct + 64).astype(np.int64)
    _, first = np.unique(drawn, return_index=True)
    drawn = drawn[np.sort(first)]                  # distinct, in the order drawn
    pool = np.concatenate([must, drawn[~np.isin(drawn, must)]])[:distinct]
    assert len(np.unique(pool)) == distinct
    return pool.astype(np.int32)


def gen_few_values(sr, distinct, width=0):
    """The pattern of float_ref.gen_few_values with `distinct` value words: the coded layouts of the tiled plan."""
    c = F.gen_few_values(distinct)
    rng = np.random.default_rng(2000 + 10 * distinct + sr)
    return case(sr, c["rows"], c["cols"], c["rp"], c["ci"], rng, pool=value_pool(rng, distinct), width=width)


def generators(clustered_matrix):
    """name -> f(sr, width) of the six one-launch input sets."""
    return {
        "ragged": gen_ragged,
        "clustered": lambda sr, width=0: gen_clustered(sr, clustered_matrix, width),
        "wide": gen_wide,
        "few16": lambda sr, width=0: gen_few_values(sr, 16, width),
        "few255": lambda sr, width=0: gen_few_values(sr, 255, width),
        "few4000": lambda sr, width=0: gen_few_values(sr, 4000, width),
    }


def all_negative(c, seed=401):
    """The (max,min) input set `c` with every value, x and y < 0: any 0 that leaks in from padding wins the max."""
    rng = np.random.default_rng(seed)
    c = dict(c)
    c["x"], c["y"] = negative_words(rng, c["cols"]), negative_words(rng, c["rows"])
    c["va"] = negative_words(rng, int(c["rp"][-1]))
    return c


def dead_tiles(c, tile, live_tiles, seed=402):
    """The input set `c` with x the identity (0, resp. INT_MIN) in every column tile of `tile` columns except
    `live_tiles`; the values keep their wide words.  The tiled plan skips a tile whose x words all absorb."""
    c = dict(c)
    x = np.full(c["cols"], 0 if c["sr"] == OR_AND else INT_MIN, np.int32)
    for t in live_tiles:
        x[t * tile:(t + 1) * tile] = c["x"][t * tile:(t + 1) * tile]
    c["x"] = x
    return c


# ------------------------------------------------------------------ square matrices for the iterations
def graph(name, sr, seed=500):
    """(n, rp, ci, values) on the `ragged` or `edges` pattern of tests/graph_patterns.py with wide-word values."""
    if name == "ragged":
        rng, rp, ci = P.ragged_pattern()
    else:
        rp, ci = P.edges_pattern()
        rng = np.random.default_rng(seed)
    nnz = int(rp[-1])
    va = truth_words(rng, nnz) if sr == OR_AND else words(rng, nnz)
    return len(rp) - 1, rp, ci, va


def start(sr, n, rng, truthy=0.002):
    """x0 == y0 of an iteration.  (max,min): words().  (or,and): `truthy` of the vertices marked by wide words (not 1: the
    first launch changes every one of them to 1), INT_MIN and 0x00010000 always among the marks."""
    if sr == MAX_MIN:
        return words(rng, n)
    x0 = np.zeros(n, np.int32)
    marked = np.nonzero(rng.random(n) < truthy)[0]
    marked = np.union1d(marked, [0, n // 2])
    w = words(rng, len(marked))
    w[w == 0] = -1
    w[w == 1] = 2
    w[0], w[-1] = INT_MIN, 0x00010000
    x0[marked] = w
    return x0
