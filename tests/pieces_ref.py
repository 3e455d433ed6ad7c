"""A numpy model of the row-piece step seam (sh_spmv_step / sh_spmv_step_pieces, include/sparseharness_hip.h), plus the
named geometries and matrices that tests/test_pieces_ref.py (no GPU) and tests/test_pieces_gpu.py share.

The seam adds three things to an ordinary launch and the model restates each:
  geometry         row r of the matrix lives in piece c = r // piece_rows and is element
                   element_of_piece[c] + (r - c * piece_rows) of out, of y and -- for the convergence test -- of x;
  expected_out     what the whole out vector holds after a launch: the row values at the rows' elements, the word that
                   was there before everywhere else (nobody writes between the pieces);
  expected_changed `differs` of csrc/semiring.hip.h per row: floats not (float64(abs(float32(in - out))) < delta), so a
                   NaN differs; ints !=.  The changed word of a launch is the OR over the rows.

`rule` selects deliberately broken models ("le": <= in place of <; "last-delta": the last piece's offset ignored) that
tests/test_pieces_ref.py shows to fail the assertions the right model passes.
"""
import numpy as np

from sparseharness_amd import partition

PLUS_TIMES_F32, MIN_PLUS_F32, OR_AND_I32, MAX_MIN_I32 = 0, 1, 2, 3
SEMIRINGS = (PLUS_TIMES_F32, MIN_PLUS_F32, OR_AND_I32, MAX_MIN_I32)
FLT_MAX = np.float32(3.4028235e38)
INT_MIN = -2 ** 31
MAX_PIECES = 8
SENTINEL = 0xDEADBEEF   # a word no row value of the tests' data has (as float: -6.26e18, not a NaN)


def elem_dtype(sr):
    return np.int32 if sr in (OR_AND_I32, MAX_MIN_I32) else np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ the model
def geometry(rows, n_pieces, piece_rows, element_of_piece, rule="right"):
    """For every row, its element (int64[rows])."""
    assert 1 <= n_pieces <= MAX_PIECES and piece_rows >= 1 and n_pieces * piece_rows >= rows
    r = np.arange(rows, dtype=np.int64)
    c = r // piece_rows
    at = np.asarray(list(element_of_piece)[:n_pieces], np.int64)[c] + (r - c * piece_rows)
    if rule == "last-delta":
        at = np.where(c == n_pieces - 1, r, at)
    return at


def expected_out(sentinel_vector, row_values, geom):
    """The whole out vector: the sentinel kept wherever no row lives."""
    out = np.array(sentinel_vector, copy=True)
    assert len(np.unique(geom)) == len(geom)
    out[geom] = np.ascontiguousarray(row_values).view(out.dtype)
    return out


def expected_changed(sr, prev, out, delta, rule="right"):
    """Per row: does the convergence test fail?  prev / out are the rows' words of the previous and the new vector."""
    if sr in (OR_AND_I32, MAX_MIN_I32):
        return np.asarray(prev, np.int32) != np.asarray(out, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs((np.asarray(prev, np.float32) - np.asarray(out, np.float32)).astype(np.float32)).astype(np.float64)
        return ~((d <= delta) if rule == "le" else (d < delta))


# ------------------------------------------------------------------ named geometries
class Geometry:
    """n_pieces pieces of piece_rows rows at `elements`; `length` = the shortest vector that holds them; `at` = the
    model's row -> element map; rows_of(c) = (first row, row count) of piece c."""

    def __init__(self, name, rows, n_pieces, piece_rows, elements, length, base=0):
        self.name, self.rows, self.n_pieces, self.piece_rows = name, rows, n_pieces, piece_rows
        self.elements = [int(e) + base for e in elements]
        self.length = int(length) + base
        self.at = geometry(rows, n_pieces, piece_rows, self.elements)
        for c in range(n_pieces):
            lo, n = self.rows_of(c)
            assert self.elements[c] >= 0 and self.elements[c] + n <= self.length

    def rows_of(self, c):
        lo = min(self.rows, c * self.piece_rows)
        return lo, min(self.rows, (c + 1) * self.piece_rows) - lo

    def boundary_rows(self):
        """First and last row of the matrix and of every piece that holds rows."""
        b = set()
        for c in range(self.n_pieces):
            lo, n = self.rows_of(c)
            if n:
                b.update((lo, lo + n - 1))
        return sorted(b)


def rank1of2x3_layout(rows):
    """The layout classes' answer for rank 1 of 2 with 3 chunks, when rank 1 owns `rows` rows and rank 0 a few more."""
    r0 = rows + rows // 3 + 37
    return partition.SlottedLayout([0, r0, r0 + rows], 3)


_GAPS = (3, 64, 1, 17, 5, 130, 2, 9)


def named_geometry(name, rows, base=0):
    """base: added to every element (the GPU tests of the changed word keep the pieces behind the matrix' columns)."""
    if name == "identity":
        return Geometry(name, rows, 1, max(rows, 1), [0], rows, base)
    if name == "rank1of2x3":
        lay = rank1of2x3_layout(rows)
        return Geometry(name, rows, 3, max(lay.piece, 1), [lay.piece_offset(1, c) for c in range(3)], lay.length, base)
    if name == "eight_odd":
        # 8 pieces of an odd number of rows, placed in DESCENDING element order with unequal gaps, the lowest at 7
        p = -(-max(rows, 1) // 8) | 1
        el = [0] * 8
        el[7] = 7
        for c in range(6, -1, -1):
            el[c] = el[c + 1] + p + _GAPS[c]
        return Geometry(name, rows, 8, p, el, el[0] + p + 11, base)
    if name == "overcover":
        # 6 pieces of which two hold all rows; the four empty ones point at the very end, at element 0 and into piece 0
        p = rows // 2 + 3
        length = 5 + 2 * p + 13 + 6
        return Geometry(name, rows, 6, p, [5, 5 + p + 13, length, 0, 6, length - 1], length, base)
    if name == "inside_bin":
        # piece boundaries one row behind a multiple of the tiled plan's row bins (2048 rows)
        k = max(1, -(-rows // (MAX_PIECES * 2048)))
        p = 2048 * k + 1
        n = max(1, -(-rows // p))
        return Geometry(name, rows, n, p, [2 + c * (p + 5) for c in range(n)], 2 + n * (p + 5), base)
    raise KeyError(name)


GEOMETRIES = ("identity", "rank1of2x3", "eight_odd", "overcover", "inside_bin")


# ------------------------------------------------------------------ named matrices
# Row length classes of the engine's row reduction (csrc/kernels.hip.h) and of its plans: one lane (<= 40), 8 lanes
# (<= 256), 64 lanes and still light under the tiled plan (< 512 at up to 64 column tiles), heavy under the tiled plan,
# above SEG_NNZ = 8192 (the CSR-stream plan's long-row fix-up).
MIXED_ROWS, MIXED_COLS = 40_000, 100_000
MIXED_CLASS_ROWS = {"empty": 1000, "one_lane": 1001, "eight_lanes": 1024, "sixty_four_lanes": 1152, "heavy": 11_111,
                    "long": 23_456}
MANY_ROWS, MANY_COLS = 620_000, 1_300_000
_cache = {}


def _mixed_lengths():
    r = np.arange(MIXED_ROWS)
    deg = (r * 7919) % 41                       # 0..40: empty rows and one-lane rows
    deg[r % 64 == 0] = 41 + (r[r % 64 == 0] // 64 * 37) % 216       # 41..256
    deg[r % 128 == 0] = 257 + (r[r % 128 == 0] // 128 * 29) % 255   # 257..511
    deg[[3333, 11_111, 17_777, 26_000, 31_999, 38_001]] = [3000, 3001, 2999, 3003, 3000, 3002]
    deg[23_456] = 20_001
    deg[1000], deg[1001], deg[1024], deg[1152] = 0, 40, 256, 511
    for g in GEOMETRIES:                        # first and last row of the matrix and of every piece: not empty
        for b in named_geometry(g, MIXED_ROWS).boundary_rows():
            deg[b] = max(deg[b], 1 + b % 3)
    return deg


def _csr(name, deg, cols, seed):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    if nnz:
        oob = rng.random(nnz) < 0.01
        ci[oob] = rng.choice(np.array([-1, cols, cols + 5], np.int32), int(oob.sum()))
    k = rng.integers(1, 301, nnz)
    vf = (k / 64.0).astype(np.float32)          # multiples of 1/64 below 4.7
    vi = (k - 6).astype(np.int32)               # zeros and negative words among them
    return {"name": name, "rows": len(deg), "cols": cols, "rp": rp, "ci": ci, "vf": vf, "vi": vi}


def matrix(name):
    """{"rows", "cols", "rp", "ci", "vf" (float32 values), "vi" (int32 values)}; built once per process."""
    if name not in _cache:
        if name == "mixed":
            m = _csr(name, _mixed_lengths(), MIXED_COLS, 11)
        elif name == "all_heavy":
            m = _csr(name, np.full(6, 3000), 100_000, 12)
        elif name == "many_bins":
            deg = np.array([4, 3, 5, 0, 4, 6, 2, 8])[np.arange(MANY_ROWS) % 8]
            deg[[0, 77_777, 310_001, MANY_ROWS - 1]] = [5, 3000, 3001, 2]
            m = _csr(name, deg, MANY_COLS, 13)
        elif name == "mixed_far":
            # `mixed` with every column moved behind the first `rows` elements of x: x[0 .. rows) is then free to hold a
            # previous vector (sh_spmv_step at x_row_offset = 0) without changing the product
            m = dict(matrix("mixed"), name=name)
            ci, rows, cols = m["ci"], m["rows"], m["cols"]
            inside = (ci >= 0) & (ci < cols)
            m["ci"] = np.where(inside, rows + ci % (cols - rows), ci).astype(np.int32)
        elif name == "tiny":
            m = _csr(name, np.zeros(10, np.int64), 10, 14)
        else:
            raise KeyError(name)
        _cache[name] = m
    return _cache[name]


def values(m, sr):
    return m["vi"] if sr in (OR_AND_I32, MAX_MIN_I32) else m["vf"]


# alpha, beta of the launches: every epilogue reads y
SCALARS = {PLUS_TIMES_F32: (2.0, 1.0), MIN_PLUS_F32: (0.25, 0.5), OR_AND_I32: (1, 1), MAX_MIN_I32: (1000, -3)}


def vector(sr, n, seed):
    """An input vector: floats in {0, 1, 3} (every partial sum of k/64 * x is exact in float), the (min,+) ones with
    a third FLT_MAX; (or,and) words in {0, 1, 3}, five in six of them 0 so that the rows' 0 / 1 results vary; (max,min)
    words around zero with INT_MIN among them."""
    rng = np.random.default_rng(1000 * seed + sr)
    v = rng.choice(np.array([0, 1, 3]), n)
    if sr == PLUS_TIMES_F32:
        return v.astype(np.float32)
    if sr == MIN_PLUS_F32:
        return np.where(rng.random(n) < 1 / 3, FLT_MAX, v.astype(np.float32)).astype(np.float32)
    if sr == OR_AND_I32:
        return np.where(rng.random(n) < 0.75, 0, v).astype(np.int32)
    w = rng.integers(-9, 60, n).astype(np.int32)
    w[rng.random(n) < 0.05] = INT_MIN
    return w


def exact_in_float(m, x):
    """Is every (+,x) row sum of m's float values with this x exact whatever the order?  All terms are multiples of
    1/64 and non-negative: yes while the largest row sum stays below 2^24 / 64."""
    ci, cols = m["ci"], m["cols"]
    ok = (ci >= 0) & (ci < cols)
    term = np.where(ok, x[np.clip(ci, 0, cols - 1)].astype(np.float64), 0.0) * m["vf"].astype(np.float64)
    sums = np.add.reduceat(np.concatenate([term, [0.0]]), np.minimum(m["rp"][:-1], len(term)))
    sums[np.diff(m["rp"]) == 0] = 0
    return bool(sums.max(initial=0.0) < 2 ** 24 / 64 - 64)


# ------------------------------------------------------------------ the changed word: fixed points and one row off
# alpha, beta when y ALIASES the previous vector: with these the epilogue is idempotent in y for the order-free
# semirings -- kernel(x, y = kernel(x, y0)) == kernel(x, y0) -- and dot is a fixed point of 0.5 * dot + 0.5 * y.
ALIAS_SCALARS = {PLUS_TIMES_F32: (0.5, 0.5), MIN_PLUS_F32: (0.25, 0.0), OR_AND_I32: (1, 1), MAX_MIN_I32: (1000, -3)}


def row_values(m, sr, x, yrow, alpha, beta):
    """oracle.kernel over the whole matrix; x covers the columns, yrow holds one word per row."""
    from oracle import oracle as O
    return O.kernel(sr, m["rp"], m["ci"], values(m, sr), x[:m["cols"]], yrow, alpha, beta, vlength=m["cols"])


def one_row_value(m, sr, x, r, yword, alpha, beta):
    """oracle.kernel for row r alone with y[r] = yword."""
    from oracle import oracle as O
    s, e = int(m["rp"][r]), int(m["rp"][r + 1])
    rp = np.array([0, e - s], np.int32)
    y = np.array([yword], elem_dtype(sr))
    return O.kernel(sr, rp, m["ci"][s:e], values(m, sr)[s:e], x[:m["cols"]], y, alpha, beta, vlength=m["cols"])[0]


def fixed_point(m, sr, x):
    """A previous vector (one word per row) that a launch with y aliasing it, under ALIAS_SCALARS, reproduces: the
    rows' own dots through the epilogue (y0 = the semiring's identity), so that a word set higher is pulled back."""
    a, b = ALIAS_SCALARS[sr]
    if sr == PLUS_TIMES_F32:
        return row_values(m, sr, x, np.zeros(m["rows"], np.float32), 1.0, 0.0)
    y0 = {MIN_PLUS_F32: FLT_MAX, OR_AND_I32: 0, MAX_MIN_I32: INT_MIN}[sr]
    return row_values(m, sr, x, np.full(m["rows"], y0, elem_dtype(sr)), a, b)


def perturbed(sr, word):
    """Another word than `word`, at least 1 away (the tests' delta is 0.25)."""
    if sr in (PLUS_TIMES_F32, MIN_PLUS_F32):
        return np.float32(word + 1.0) if word < 1e30 else np.float32(2.0)
    if sr == OR_AND_I32:
        return np.int32(0 if word else 1)
    return np.int32(word + 1) if word < 2 ** 31 - 1 else np.int32(word - 1)
