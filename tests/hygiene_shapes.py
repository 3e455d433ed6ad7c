"""Inputs for the launch-hygiene tests: what a launch may read is its operands and what it wrote itself.  CPU only: numpy
and the C oracle; nothing here touches the engine.  Not a test and not a conftest.  tests/test_hygiene_cpu.py proves from
the references alone that these inputs make a stale or foreign scratch word visible; tests/test_hygiene_gpu.py runs the
engine on them.

The poison of a semiring is the word that dominates its reduction: folded into a row's sum it decides the row.
(+,x): a quiet NaN.  (min,+): +0.0 -- which is also what fresh device memory usually holds.  (or,and): all ones.
(max,min): INT_MAX, under alpha = INT_MAX.  `visible` says, per row, whether the output word changes when the poison
joins the reduction; the epilogues are chosen so that it does for every row of three semirings and for every row whose
(or,and) result is 0.

Shapes, the smallest that reach every scratch array:
  "tiled3": 5000 rows (three row bins of 2048), 3 * 32760 - 1001 columns (three column tiles, the last one partial,
            cols % 4 == 3), Poisson(8) rows, 60 rows of 150 entries (pairs fold), two heavy rows of 3000 entries.
  "tiled2": the same rows over exactly 2 * 32760 columns: every tile is a full one.
  "stream": the square ragged pattern of graph_patterns.ragged_pattern(): one row of 20 001 entries (three long-row
            segments and the fix-up), columns out of range on both sides.  That row reads nearly every column, so under
            (or,and) its result is 0 -- and a poison visible in it -- under x_0 only.
All data is integer-valued and small enough that every (+,x) sum is below 2^24: exact in any order, so every comparison
is == on the 32-bit words.

Liveness, per column tile (per third of the columns on "stream"): x_A is live in tiles {0, 2}, x_B in tile {1} only,
x_0 nowhere; elsewhere x holds the semiring's absorbing word.  The sequence A, B, 0, A, B takes every tile through
live -> dead -> live on one handle.  ("tiled2" has no tile 2: A is tile 0, B is tile 1.)"""
import functools

import numpy as np

import graph_patterns as G
from oracle import oracle as O

PT, MP, OA, MM = O.PLUS_TIMES_F32, O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32
SEMIRINGS = (PT, MP, OA, MM)
SR_NAME = {PT: "plus_times", MP: "min_plus", OA: "or_and", MM: "max_min"}
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
TCOLS, TBIN_ROWS = 32760, 2048
POISON = {PT: 0x7FC00000, MP: 0x00000000, OA: 0xFFFFFFFF, MM: 0x7FFFFFFF}
ABSORBING = {PT: np.float32(0.0), MP: O.FLT_MAX, OA: np.int32(0), MM: np.int32(INT_MIN)}
SCALARS = {PT: (1.0, 0.5), MP: (0.0, 0.0), OA: (1, 1), MM: (INT_MAX, 5)}
NEUTRAL = {PT: (1.0, 0.0), MP: (0.0, 0.0), OA: (1, 0), MM: (INT_MAX, INT_MIN)}   # epilogues that hand the row sum through
SEQUENCE = ("A", "B", "0", "A", "B")
VALUE_SETS = {"nibble16": (16, 4), "byte255": (255, 8), "short4000": (4000, 16), "raw": (5000, 0)}   # distinct values, code bits
HEAVY_ROWS = (1700, 4100)
TILED = {"tiled3": 3 * TCOLS - 1001, "tiled2": 2 * TCOLS}
SHAPES = ("tiled3", "tiled2", "stream")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def is_int(sr):
    return sr in (OA, MM)


# ------------------------------------------------------------------ patterns
@functools.lru_cache(maxsize=None)
def pattern(shape):
    """-> (rows, cols, rp, ci)."""
    if shape == "stream":
        _, rp, ci = G.ragged_pattern()
        n = len(rp) - 1
        return (n, n) + frozen(rp, ci)
    cols = TILED[shape]
    rng = np.random.default_rng(9000 + cols)
    rows = 5000
    deg = rng.poisson(8, rows).astype(np.int64)
    deg[rng.choice(rows, 40, replace=False)] = 0
    deg[rng.choice(np.arange(700, rows), 60, replace=False)] = 150
    for h in HEAVY_ROWS:
        deg[h] = 3000
    deg[0], deg[rows - 1] = 9, 9
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, cols, int(rp[-1])).astype(np.int32)
    ci[0], ci[rp[rows] - 1] = 0, cols - 1               # the first and the last column are read
    ci[rp[rows - 1]] = cols - 2
    return (rows, cols) + frozen(rp, ci)


def segment_of(shape):
    """The columns of one liveness segment: a column tile, or a third of the stream shape's columns."""
    return TCOLS if shape in TILED else (pattern(shape)[1] + 2) // 3


@functools.lru_cache(maxsize=None)
def heavy_columns(shape):
    """Columns that a heavy (tiled) or long (stream) row reads."""
    rows, cols, rp, ci = pattern(shape)
    heavy = np.nonzero(np.diff(rp) >= 3000)[0]
    m = np.zeros(cols, bool)
    for h in heavy:
        c = ci[rp[h]:rp[h + 1]]
        m[c[(c >= 0) & (c < cols)]] = True
    return frozen(heavy, m)


@functools.lru_cache(maxsize=None)
def values(shape, vset):
    """Small positive integers, `distinct` different ones, each occurring: the first `distinct` entries (light rows in
    front of the first heavy row) hold 1 .. distinct, every other entry a value of 1 .. 16."""
    distinct = VALUE_SETS[vset][0]
    rows, cols, rp, ci = pattern(shape)
    nnz = len(ci)
    rng = np.random.default_rng(9100 + distinct)
    v = rng.integers(1, 17, nnz).astype(np.int64)
    first_big = int(rp[np.nonzero(np.diff(rp) >= 3000)[0][0]])
    assert distinct <= first_big
    v[:distinct] = 1 + np.arange(distinct)
    return frozen(v)[0]


def values_for(sr, shape, vset):
    return values(shape, vset).astype(O.elem_dtype(sr))


# ------------------------------------------------------------------ vectors
@functools.lru_cache(maxsize=None)
def x_vector(sr, shape, which):
    """which: "A" live in segments {0, 2}, "B" in segment {1}, "0" all absorbing."""
    rows, cols, rp, ci = pattern(shape)
    seg = np.arange(cols) // segment_of(shape)
    live = {"A": (seg == 0) | (seg == 2), "B": seg == 1, "0": np.zeros(cols, bool)}[which]
    rng = np.random.default_rng(9200 + 10 * sr + ord(which))
    if sr == PT:
        x = np.where(live, 1 + np.arange(cols) % 7, 0)
    elif sr == MP:
        x = np.where(live, np.arange(cols) % 11, 0)
    elif sr == OA:
        # sparse, and outside the heavy rows' columns: most rows, and both heavy rows, have the result 0 that a poison shows in
        # (the stream shape's long row reads nearly every column: only x_0 leaves its result 0)
        live = live & (rng.random(cols) < 0.02)
        if shape in TILED:
            live &= ~heavy_columns(shape)[1]
        x = np.where(live, 1 + np.arange(cols) % 5, 0)
    else:
        x = np.where(live, 1 + np.arange(cols) % 1000, 0)
    x = x.astype(O.elem_dtype(sr))
    x[~live] = ABSORBING[sr]
    if which != "0":
        assert live[seg == (1 if which == "B" else 0)].any()
    return frozen(x)[0]


@functools.lru_cache(maxsize=None)
def y_vector(sr, rows):
    """(min,+): no word is 0 (so that a 0 from a poisoned sum shows), most are FLT_MAX (so that the sum decides)."""
    r = np.arange(rows)
    if sr == PT:
        y = (r % 5).astype(np.float32)
    elif sr == MP:
        y = np.where(r % 5 == 0, 1 + r % 9, O.FLT_MAX).astype(np.float32)
    elif sr == OA:
        y = (r % 7 == 0).astype(np.int32)
    else:
        y = (r % 9 - 4).astype(np.int32)
    return frozen(y)[0]


# ------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def want(sr, shape, vset, which):
    """O.kernel under SCALARS[sr]."""
    rows, cols, rp, ci = pattern(shape)
    return frozen(O.kernel(sr, rp, ci, values_for(sr, shape, vset), x_vector(sr, shape, which), y_vector(sr, rows), *SCALARS[sr]))[0]


@functools.lru_cache(maxsize=None)
def row_sums(sr, shape, vset, which):
    """The reduction of every row before the epilogue, by the oracle under an epilogue that hands it through."""
    rows, cols, rp, ci = pattern(shape)
    y = np.full(rows, {PT: 0.0, MP: O.FLT_MAX, OA: 0, MM: INT_MIN}[sr], O.elem_dtype(sr))
    return frozen(O.kernel(sr, rp, ci, values_for(sr, shape, vset), x_vector(sr, shape, which), y, *NEUTRAL[sr]))[0]


def epilogue(sr, acc, y, alpha, beta):
    """The oracle's epilogues (oracle/sh_oracle.c) on numpy arrays."""
    if sr == PT:
        with np.errstate(invalid="ignore"):
            return (acc * np.float32(alpha) + y * np.float32(beta)).astype(np.float32)
    if sr == MP:
        with np.errstate(over="ignore"):
            return np.minimum(np.abs(acc) + np.float32(abs(alpha)), np.abs(y) + np.float32(abs(beta))).astype(np.float32)
    if sr == OA:
        return (((acc != 0) & (alpha != 0)) | ((y != 0) & (beta != 0))).astype(np.int32)
    return np.maximum(np.minimum(acc, np.int32(alpha)), np.minimum(y, np.int32(beta))).astype(np.int32)


def fold_poison(sr, acc):
    """add(acc, poison) of the semiring, per row."""
    p = np.array([POISON[sr]], np.uint32).view(O.elem_dtype(sr))[0]
    if sr == PT:
        return (acc + p).astype(np.float32)
    if sr == MP:
        return np.minimum(np.abs(acc), np.abs(p)).astype(np.float32)
    if sr == OA:
        return ((acc != 0) | (p != 0)).astype(np.int32)
    return np.maximum(acc, p).astype(np.int32)


def visible_xy(sr, shape, vset, x, y):
    """Per row, for any x and y: the output word changes when the poison joins the row's reduction.  -> (visible, clean)."""
    rows, cols, rp, ci = pattern(shape)
    va = values_for(sr, shape, vset)
    neutral_y = np.full(rows, {PT: 0.0, MP: O.FLT_MAX, OA: 0, MM: INT_MIN}[sr], O.elem_dtype(sr))
    acc = O.kernel(sr, rp, ci, va, x, neutral_y, *NEUTRAL[sr])
    clean = epilogue(sr, acc, y, *SCALARS[sr])
    assert np.array_equal(bits(clean), bits(O.kernel(sr, rp, ci, va, x, y, *SCALARS[sr]))), "the numpy epilogue is not the oracle's"
    return bits(epilogue(sr, fold_poison(sr, acc), y, *SCALARS[sr])) != bits(clean), clean


def visible(sr, shape, vset, which):
    """Per row: the output word changes when the poison joins the row's reduction.  From the reference alone."""
    rows = pattern(shape)[0]
    vis, clean = visible_xy(sr, shape, vset, x_vector(sr, shape, which), y_vector(sr, rows))
    assert np.array_equal(bits(clean), bits(want(sr, shape, vset, which)))
    return vis


# ------------------------------------------------------------------ several vectors per launch (stream shape)
STREAM_HUB = 7   # the column that most rows of the stream shape read (graph_patterns.ragged_pattern)


def rolled_x(sr, which, j):
    """x_A / x_B / x_0 of the stream shape rotated by j columns.  Under (or,and) the hub column stays 0: a live word there
    would set most rows to 1 and hide a poison in them."""
    x = np.roll(x_vector(sr, "stream", which), j)
    if sr == OA:
        x[STREAM_HUB] = 0
    return x


def column_of(sr, k, j):
    """Column j of the k-th launch of the sequence: the x of launch k + j, rotated by j columns."""
    return rolled_x(sr, SEQUENCE[(k + j) % len(SEQUENCE)], j)


def y_column_of(sr, j):
    return np.roll(y_vector(sr, pattern("stream")[0]), j)


@functools.lru_cache(maxsize=None)
def spmm_case(sr, width, k):
    """-> (X (cols, width), Y (rows, width), want (rows, width)) of launch k of the sequence, vset "nibble16"."""
    rows, cols, rp, ci = pattern("stream")
    va = values_for(sr, "stream", "nibble16")
    X = np.ascontiguousarray(np.stack([column_of(sr, k, j) for j in range(width)], axis=1))
    Y = np.ascontiguousarray(np.stack([y_column_of(sr, j) for j in range(width)], axis=1))
    W = np.stack([O.kernel(sr, rp, ci, va, X[:, j].copy(), Y[:, j].copy(), *SCALARS[sr]) for j in range(width)], axis=1)
    return frozen(X, Y, np.ascontiguousarray(W))


def pack(M, words):
    """(n, 32 * words) truth values -> (n, words) uint32: source s = bit s % 32 of word s // 32."""
    n = M.shape[0]
    out = np.zeros((n, words), np.uint32)
    for s in range(32 * words):
        out[:, s // 32] |= (M[:, s] != 0).astype(np.uint32) << np.uint32(s % 32)
    return out


BITS_DISTINCT = 8   # distinct columns among the sources of a packed launch (source s holds column s % 8)


@functools.lru_cache(maxsize=None)
def bits_case(words, k):
    """-> (X (cols, words), Y (rows, words), want (rows, words)) packed, of launch k of the sequence; alpha = beta = 1."""
    rows, cols, rp, ci = pattern("stream")
    va = values_for(OA, "stream", "nibble16")
    xs = [column_of(OA, k, j) for j in range(BITS_DISTINCT)]
    ys = [y_column_of(OA, j) for j in range(BITS_DISTINCT)]
    ws = [O.kernel(OA, rp, ci, va, xs[j], ys[j], 1, 1) for j in range(BITS_DISTINCT)]
    pick = [s % BITS_DISTINCT for s in range(32 * words)]
    return frozen(*(pack(np.stack([v[j] for j in pick], axis=1), words) for v in (xs, ys, ws)))


# ------------------------------------------------------------------ the loops: a path with chords
LOOP_N, LOOP_CHORD = 2000, 40
LOOP_SOURCES = (0, 3, 41, 500, 999, 1500, 1960, 1999)
LOOP_SCALARS = {MP: (0.0, 0.0), OA: (1, 1), MM: (1 << 30, 1 << 30)}
LOOP_CAP = 1000
DELTA = 1e-4


@functools.lru_cache(maxsize=None)
def loop_graph():
    """Vertex i reads vertices i - 1 and i - 40: from vertex 0 the last vertex is 49 + 39 hops away, so every loop
    needs more than ten batches of eight launches."""
    r = np.arange(LOOP_N)
    pairs = [(i, i - d) for i in r for d in (1, LOOP_CHORD) if i - d >= 0]
    rows_, cols_ = np.array(pairs).T
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows_, minlength=LOOP_N))]).astype(np.int32)
    return (LOOP_N,) + frozen(rp, cols_.astype(np.int32))


def loop_values(sr):
    n, rp, ci = loop_graph()
    return {MP: lambda: 1.0 + (np.arange(len(ci)) % 3), OA: lambda: np.ones(len(ci)), MM: lambda: np.full(len(ci), 1 << 20)}[sr]().astype(O.elem_dtype(sr))


@functools.lru_cache(maxsize=None)
def loop_start(sr, v):
    n = LOOP_N
    if sr == MP:
        x = np.full(n, O.FLT_MAX, np.float32)
        x[v] = 0.0
    elif sr == OA:
        x = np.zeros(n, np.int32)
        x[v] = 1
    else:   # the largest label, at v, runs down the graph
        x = np.full(n, -1, np.int32)
        x[v] = 1000
    return frozen(x)[0]


@functools.lru_cache(maxsize=None)
def loop_ref(sr, v):
    """O.iterate from source v, y0 = x0 -> (vector, launches, converged)."""
    n, rp, ci = loop_graph()
    x0 = loop_start(sr, v)
    x, it, conv = O.iterate(sr, rp, ci, loop_values(sr), x0, x0, *LOOP_SCALARS[sr], DELTA, LOOP_CAP)
    return frozen(x)[0], it, conv


@functools.lru_cache(maxsize=None)
def loop_levels(v):
    """newly_set of the (or,and) source v: vertices switched on by launch l, one O.kernel launch at a time."""
    n, rp, ci = loop_graph()
    va, x0 = loop_values(OA), loop_start(OA, v)
    x, sizes = x0, []
    for _ in range(loop_ref(OA, v)[1]):
        nxt = O.kernel(OA, rp, ci, va, x, x0, 1, 1)
        sizes.append(int(((x == 0) & (nxt != 0)).sum()))
        x = nxt
    return tuple(sizes)


# ------------------------------------------------------------------ sh_iterate on the stream shape
STREAM_SOURCE, STREAM_CAP = 11, 40


@functools.lru_cache(maxsize=None)
def stream_loop(sr):
    """sh_iterate on the stream shape (square; the long row's segments and fix-up run in every launch), one source,
    y0 = x0 -> (values, x0, vector, launches, converged) by O.iterate under LOOP_SCALARS, stopped at STREAM_CAP."""
    n, _, rp, ci = pattern("stream")
    va = np.where(values("stream", "nibble16") > 0, {MP: 1, OA: 1, MM: 1 << 20}[sr], 0) * (1 + (np.arange(len(ci)) % 3 if sr == MP else 0))
    va = va.astype(O.elem_dtype(sr))
    x0 = np.full(n, {MP: O.FLT_MAX, OA: 0, MM: -1}[sr], O.elem_dtype(sr))
    x0[STREAM_SOURCE] = {MP: 0.0, OA: 1, MM: 1000}[sr]
    x, it, conv = O.iterate(sr, rp, ci, va, x0, x0, *LOOP_SCALARS[sr], DELTA, STREAM_CAP)
    return frozen(va, x0, x) + (it, conv)


# ------------------------------------------------------------------ sh_iterate over three column tiles
LONG_N, LONG_CHORD, LONG_CAP = 2 * TCOLS + 3, 1000, 20
LONG_SOURCES = (5, TCOLS - 2, TCOLS + 1, 2 * TCOLS - 2, 2 * TCOLS + 1)   # on both sides of each tile seam, and in the last three columns
LONG_BACKGROUND = {MP: O.FLT_MAX, OA: 0, MM: -1}


@functools.lru_cache(maxsize=None)
def long_path():
    """A path of 2 * 32760 + 3 vertices with chords of 1000 (vertex i reads i - 1 and i - 1000): two full column tiles
    and one of three columns."""
    n = LONG_N
    i = np.arange(1, n)
    rows_ = np.concatenate([i, i[i >= LONG_CHORD]])
    cols_ = np.concatenate([i - 1, i[i >= LONG_CHORD] - LONG_CHORD])
    order = np.lexsort((cols_, rows_))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows_, minlength=n))]).astype(np.int32)
    return (n,) + frozen(rp, cols_[order].astype(np.int32))


@functools.lru_cache(maxsize=None)
def long_case(sr):
    """-> (values, x0): a source on both sides of each tile seam and in the last tile, so that every tile of every
    launch's input holds words that are not the background (tests/test_hygiene_cpu.py asserts it)."""
    n, rp, ci = long_path()
    va = np.full(len(ci), {MP: 1.0, OA: 1, MM: 1 << 20}[sr], O.elem_dtype(sr))
    x0 = np.full(n, LONG_BACKGROUND[sr], O.elem_dtype(sr))
    for q, v in enumerate(LONG_SOURCES):
        x0[v] = {MP: float(q), OA: 1, MM: 1000 + q}[sr]
    return frozen(va, x0)


@functools.lru_cache(maxsize=None)
def long_ref(sr):
    n, rp, ci = long_path()
    va, x0 = long_case(sr)
    x, it, conv = O.iterate(sr, rp, ci, va, x0, x0, *LOOP_SCALARS[sr], DELTA, LONG_CAP)
    return frozen(x)[0], it, conv
