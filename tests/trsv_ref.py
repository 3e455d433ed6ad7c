"""The definition of sh_trsv (include/sparseharness_hip.h) restated in numpy, the exact solve in fractions for the small
cases, the plan of runs, the footprint formula and the CASES that tests/test_trsv_ref.py (CPU: against the host gold and
the rounding bound) and tests/test_trsv_gpu.py (against the device) share.  Not a test and not a conftest.  It shares no
code with the device or with host/src/trsv_solve.cpp."""
import functools
from fractions import Fraction

import numpy as np

LANE, PIECE = 8, 2048            # TRSV_LANE, TRSV_PIECE
RUN, THIN, THIN_MAX = 1024, 256, 1 << 16
MAX_BLOCKS, BATCH, CTL_BYTES = 1024, 32, 1024


def constants():
    return dict(TRSV_LANE=LANE, TRSV_PIECE=PIECE, TRSV_BATCH=BATCH, TRSV_MAX_BLOCKS=MAX_BLOCKS, TRSV_CTL_BYTES=CTL_BYTES,
                TRSV_THIN=THIN, TRSV_THIN_MAX=THIN_MAX)


def header_footprint(rows, entries, levels):
    return 4 * (rows + 1) + 24 * rows + 8 * entries + 4 * (levels + 1) + 17408


def csr(n, entries):
    """(n, row_ptr, col_idx, val) from (r, c, v) triples; inside a row the entries keep the order given."""
    entries = list(entries)
    r = np.array([e[0] for e in entries], np.int64)
    o = np.argsort(r, kind="stable")
    rp = np.zeros(n + 1, np.int32)
    if len(entries):
        rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    ci = np.array([entries[i][1] for i in o], np.int32)
    va = np.array([entries[i][2] for i in o], np.float32)
    return n, rp, ci, va


def csr_arrays(n, r, c, v):
    """The same from arrays (stable by row)."""
    r = np.asarray(r, np.int64)
    o = np.argsort(r, kind="stable")
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return n, rp, np.asarray(c, np.int32)[o], np.asarray(v, np.float32)[o]


def transposed(mat):
    n, rp, ci, va = mat
    r = np.repeat(np.arange(n), np.diff(rp))
    keep = (ci >= 0) & (ci < n)   # (a column outside the matrix has no row to go to)
    return csr_arrays(n, ci[keep], r[keep], va[keep])


# ---- the definition
def lists(mat, uplo, unit):
    """-> (ptr, col, val, d): LIST(r) = col/val[ptr[r]:ptr[r + 1]] in ascending (column, position as given); d float64."""
    n, rp, ci, va = mat
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    c = ci.astype(np.int64)
    inside = (c >= 0) & (c < n)
    idx = np.nonzero(inside & ((c > r) if uplo else (c < r)))[0]
    o = idx[np.lexsort((idx, c[idx], r[idx]))]
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(r[o], minlength=n)) if n else 0
    d = np.zeros(n, np.float64)
    if not unit:
        for j in np.nonzero(inside & (c == r))[0]:   # left to right, from +0.0
            d[r[j]] = d[r[j]] + np.float64(va[j])
    return ptr, c[o], va[o].astype(np.float32), d


def sum_lane(t):
    """A list of at most 8 terms, as one lane adds it."""
    assert len(t) <= LANE
    p = np.zeros(LANE, np.float64)
    p[:len(t)] = np.float64(0.0) + np.asarray(t, np.float64)
    return ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]))


def sum_pieces(t, piece=PIECE):
    """Any list, as a wave adds it: pieces, 64 strided partials from +0.0, the butterfly, the piece sums left to right."""
    t = np.asarray(t, np.float64)
    acc = np.float64(0.0)
    flip = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]
    for p0 in range(0, len(t), piece):
        part = t[p0:p0 + piece]
        partial = np.zeros(64, np.float64)
        for q in range(0, len(part), 64):
            ch = part[q:q + 64]
            partial[:len(ch)] = partial[:len(ch)] + ch
        for f in flip:
            partial = partial + partial[f]
        acc = acc + partial[0]
    return acc


def list_sum(t):
    return sum_lane(t) if len(t) <= LANE else sum_pieces(t)


def solve(mat, b, uplo=0, unit=0, f32=0):
    """-> dict(x, x64, level, lstart, entries, levels, max_list, max_width, zero_diag, first_zero)."""
    n = mat[0]
    ptr, col, val, d = lists(mat, uplo, unit)
    ln = np.diff(ptr)
    rhs = np.asarray(b, np.float32).astype(np.float64) if f32 else np.asarray(b, np.float64)
    x, level = np.zeros(n, np.float64), np.zeros(n, np.int64)
    v64 = val.astype(np.float64)
    with np.errstate(all="ignore"):
        empty = ln == 0
        x[empty] = rhs[:n][empty] - np.float64(0.0)
        if not unit:
            x[empty] = x[empty] / d[empty]
        rows = np.nonzero(~empty)[0]
        for r in (rows[::-1] if uplo else rows):
            s, e = ptr[r], ptr[r + 1]
            level[r] = level[col[s:e]].max() + 1
            v = rhs[r] - list_sum(v64[s:e] * x[col[s:e]])
            x[r] = v if unit else v / d[r]
    levels = int(level.max()) + 1 if n else 0
    width = np.bincount(level, minlength=levels) if n else np.zeros(0, np.int64)
    zero = np.nonzero(d == 0.0)[0] if not unit else np.zeros(0, np.int64)
    return dict(x=x.astype(np.float32) if f32 else x, x64=x, level=level.astype(np.int32),
                lstart=np.concatenate(([0], np.cumsum(width))).astype(np.int64), entries=int(ptr[-1]), levels=levels,
                max_list=int(ln.max()) if n else 0, max_width=int(width.max()) if n else 0, zero_diag=len(zero),
                first_zero=int(zero[0]) if len(zero) else -1)


def plan(lstart, thin=None, run=RUN):
    """-> (launches, runs, levels_in_runs): a level is thin when it holds at most `thin` rows; consecutive thin levels form
    runs of at most `run` levels; every other level is a launch of its own."""
    thin = THIN if thin is None or thin < 0 else thin
    width = np.diff(np.asarray(lstart, np.int64))
    launches = runs = in_runs = 0
    L = 0
    while L < len(width):
        if width[L] > thin:
            launches, L = launches + 1, L + 1
            continue
        k = 0
        while L + k < len(width) and k < run and width[L + k] <= thin:
            k += 1
        launches, runs, in_runs, L = launches + 1, runs + 1, in_runs + k, L + k
    return launches, runs, in_runs


# ---- exactly, for the small cases
def exact_solve(mat, b, uplo=0, unit=0):
    """x as Fractions (None from the first row on whose diagonal is zero: no solution is defined there)."""
    n = mat[0]
    ptr, col, val, d = lists(mat, uplo, unit)
    x = [None] * n
    for r in (range(n - 1, -1, -1) if uplo else range(n)):
        s = Fraction(float(b[r]))
        for j in range(ptr[r], ptr[r + 1]):
            if x[col[j]] is None:
                return x
            s -= Fraction(float(val[j])) * x[col[j]]
        if not unit and d[r] == 0.0:
            return x
        x[r] = s if unit else s / Fraction(float(d[r]))
    return x


def residual_and_scale(mat, b, x, uplo=0, unit=0, x_in=None):
    """Per row, exactly: (|b - T x|_r, (|T| |x_in|)_r, len_r) with T's diagonal the float64 d the definition gives."""
    n = mat[0]
    ptr, col, val, d = lists(mat, uplo, unit)
    xin = x if x_in is None else x_in
    out = []
    for r in range(n):
        dr = Fraction(1) if unit else Fraction(float(d[r]))
        res, scale = Fraction(float(b[r])) - dr * Fraction(float(x[r])), abs(dr) * abs(Fraction(float(xin[r])))
        for j in range(ptr[r], ptr[r + 1]):
            a = Fraction(float(val[j]))
            res -= a * Fraction(float(x[col[j]]))
            scale += abs(a) * abs(Fraction(float(xin[col[j]])))
        out.append((abs(res), scale, int(ptr[r + 1] - ptr[r])))
    return out


# ---- the cases: name -> dict(mat, uplo, unit, b)
def _rng(seed):
    return np.random.default_rng(seed)


def _vals(rng, k):
    """Drawn non-integer float32 values away from zero, both signs."""
    return (rng.uniform(0.25, 1.75, k) * rng.choice([-1.0, 1.0], k)).astype(np.float32)


def tri4_matrix():
    """All 64 strictly-lower patterns of 4 rows side by side in one block-diagonal matrix, with a diagonal."""
    rng = _rng(41)
    pairs = [(r, c) for r in range(4) for c in range(r)]
    ent = []
    for p in range(64):
        for r in range(4):
            row = [(c, float(_vals(rng, 1)[0])) for (rr, c) in pairs if rr == r and p >> pairs.index((rr, c)) & 1]
            row.append((r, float(rng.uniform(1.5, 2.5))))
            for c, v in row:
                ent.append((4 * p + r, 4 * p + c, v))
    return csr(256, ent)


def tiers_matrix():
    """4100 diagonal-only rows, one row per list length on both sides of every tier, then a row that depends on those."""
    rng = _rng(42)
    base, lens = 4100, (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 4097)
    r, c, v = [np.arange(base)], [np.arange(base)], [rng.uniform(1.0, 2.0, base)]
    for i, k in enumerate(lens):
        cols = rng.permutation(base)[:k]
        r += [np.full(k + 1, base + i)]
        c += [np.append(cols, base + i)]       # (unsorted: the handle sorts)
        v += [np.append(_vals(rng, k), 1.5)]
    last = base + len(lens)
    r += [np.full(len(lens) + 1, last)]
    c += [np.append(np.arange(base, last), last)]
    v += [np.append(_vals(rng, len(lens)), 2.0)]
    return csr_arrays(last + 1, np.concatenate(r), np.concatenate(c), np.concatenate(v))


def wide_matrix():
    """One level with more rows than a capped launch has lanes (MAX_BLOCKS * 256), one dependent level above it."""
    rng = _rng(43)
    base, top = MAX_BLOCKS * 256 + 5, 67
    deps = rng.integers(0, base, (top, 3))
    r = np.concatenate([np.arange(base + top), np.repeat(np.arange(base, base + top), 3)])
    c = np.concatenate([np.arange(base + top), deps.ravel()])
    v = np.concatenate([rng.uniform(1.0, 2.0, base + top), _vals(rng, 3 * top)])
    return csr_arrays(base + top, r, c, v)


def path_matrix(n):
    rng = _rng(44 + n)
    r = np.concatenate([np.arange(n), np.arange(1, n)])
    c = np.concatenate([np.arange(n), np.arange(n - 1)])
    v = np.concatenate([rng.uniform(1.5, 2.5, n), _vals(rng, n - 1)])
    return csr_arrays(n, r, c, v)


def widths_matrix(t):
    """Consecutive levels of t - 1, t, t + 1, 1 and t + 1 rows: every row of a level depends on rows of the level before."""
    rng = _rng(45 + t)
    widths = [t - 1, t, t + 1, 1, t + 1]
    start = np.concatenate(([0], np.cumsum(widths)))
    n = int(start[-1])
    r, c, v = [np.arange(n)], [np.arange(n)], [rng.uniform(1.5, 2.5, n)]
    for L in range(1, len(widths)):
        rows = np.arange(start[L], start[L + 1])
        for _ in range(2):
            r.append(rows)
            c.append(rng.integers(start[L - 1], start[L], len(rows)))
            v.append(_vals(rng, len(rows)))
    return csr_arrays(n, np.concatenate(r), np.concatenate(c), np.concatenate(v))


GUARD = 1.0e30   # a value that would change x visibly if an ignored entry were read


def dirt_matrix():
    """Unsorted rows, parallel entries (diagonal ones too), out-of-range columns and other-triangle entries with guard
    values, explicit zeros, a missing diagonal (row 5) and a zero diagonal (row 7: 1.5 - 1.5)."""
    n = 12
    ent = [
        (0, 0, 2.0), (0, 3, GUARD), (0, -1, GUARD), (0, n, GUARD),
        (1, 1, 0.75), (1, 0, 0.5), (1, 1, 0.5), (1, 0, -0.125),             # parallel diagonal, parallel (1, 0)
        (2, 1, 0.3), (2, 2, 1.1), (2, 0, -0.7), (2, 1, 0.9), (2, 0, 0.2),   # unsorted, parallel
        (3, 3, 3.0), (3, 0, 0.0), (3, 2, -0.0), (3, 11, GUARD),             # explicit zeros
        (4, 2, 1.25), (4, 4, -1.5), (4, 2 ** 31 - 1, GUARD), (4, -2 ** 31, GUARD),
        (5, 1, 0.6), (5, 4, -0.4),                                          # no diagonal: inf or NaN
        (6, 6, 1.0), (6, 5, 0.5),                                           # reads row 5's value
        (7, 7, 1.5), (7, 7, -1.5), (7, 3, 0.25),                            # d == 0
        (8, 8, 2.0),                                                        # b = -0.0
        (9, 9, 2.0), (9, 8, 1.0),                                           # b = inf
        (10, 10, 2.0), (10, 9, 1.0), (10, 0, 1.0),                          # b = NaN
        (11, 11, 4.0), (11, 10, 0.0), (11, 2, 0.5),                         # 0 * NaN
    ]
    return csr(n, ent)


def dirt_b():
    b = _rng(46).normal(size=12)
    b[8], b[9], b[10] = -0.0, np.inf, np.nan
    return b


def ilu_matrix(n=300):
    """An ILU-style factor pair in one matrix: unit lower plus upper with its diagonal, a few entries per row."""
    rng = _rng(47)
    r = np.concatenate([np.arange(n), rng.integers(0, n, 5 * n)])
    c = np.concatenate([np.arange(n), rng.integers(0, n, 5 * n)])
    v = np.concatenate([rng.uniform(2.0, 3.0, n), _vals(rng, 5 * n) * 0.25])
    keep = np.concatenate([np.ones(n, bool), r[n:] != c[n:]])
    o = rng.permutation(int(keep.sum()))   # (rows unsorted)
    return csr_arrays(n, r[keep][o], c[keep][o], v[keep][o])


def grid_lower(side):
    """The lower triangle (with the diagonal) of the 5-point Laplacian of a side x side grid, and the full pattern."""
    idx = np.arange(side * side).reshape(side, side)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    w = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    n = side * side
    full = csr_arrays(n, np.concatenate([u, w, np.arange(n)]), np.concatenate([w, u, np.arange(n)]),
                      np.concatenate([-np.ones(2 * len(u)), 4.0 * np.ones(n)]))
    return full


def permuted(mat, perm):
    """A[perm][:, perm]: new row k is old row perm[k]."""
    n, rp, ci, va = mat
    pos = np.empty(n, np.int64)
    pos[perm] = np.arange(n)
    r = np.repeat(np.arange(n), np.diff(rp))
    return csr_arrays(n, pos[r], pos[ci], va)


def _case(mat, uplo=0, unit=0, b=None, seed=7):
    return dict(mat=mat, uplo=uplo, unit=unit, b=_rng(seed).normal(size=max(mat[0], 1))[:mat[0]] if b is None else b)


CASES = {
    "tri4-lower": lambda: _case(tri4_matrix()),
    "tri4-lower-unit": lambda: _case(tri4_matrix(), unit=1),
    "tri4-upper": lambda: _case(transposed(tri4_matrix()), uplo=1),
    "tri4-upper-unit": lambda: _case(transposed(tri4_matrix()), uplo=1, unit=1),
    "tiers": lambda: _case(tiers_matrix()),
    "wide": lambda: _case(wide_matrix()),
    "path30": lambda: _case(path_matrix(30)),
    "path-runs": lambda: _case(path_matrix(2 * RUN + 3)),
    "path-runs-upper": lambda: _case(transposed(path_matrix(2 * RUN + 3)), uplo=1),
    "widths64": lambda: _case(widths_matrix(64)),
    "widths256": lambda: _case(widths_matrix(THIN)),
    "dirt": lambda: _case(dirt_matrix(), b=dirt_b()),
    "dirt-unit": lambda: _case(dirt_matrix(), unit=1, b=dirt_b()),
    "ilu-lower-unit": lambda: _case(ilu_matrix(), unit=1),
    "ilu-upper": lambda: _case(ilu_matrix(), uplo=1),
    "rows0": lambda: _case(csr(0, [])),
    "rows1": lambda: _case(csr(1, [(0, 0, 2.5)])),
    "rows1-empty": lambda: _case(csr(1, [])),
}
SMALL = ("tri4-lower", "tri4-lower-unit", "tri4-upper", "tri4-upper-unit", "path30", "widths64", "ilu-lower-unit", "ilu-upper",
         "rows1")   # the cases the exact bound is checked on (finite, no zero diagonal)
NAN_CASES = ("dirt", "dirt-unit", "rows1-empty")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name, f32=0):
    c = case(name)
    return solve(c["mat"], c["b"], c["uplo"], c["unit"], f32)
