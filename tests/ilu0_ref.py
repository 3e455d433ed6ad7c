"""The definition of sh_ilu0 (include/sparseharness_hip.h) restated in numpy, the same recurrence in fractions for the
small cases, the plan of a call, the footprint formula and the CASES that tests/test_ilu0_ref.py (CPU: against the host
gold, exactly and in fractions) and tests/test_ilu0_gpu.py (against the device) share.  Not a test and not a conftest.
It shares no code with the device or with host/src/ilu0_factor.cpp: the slot of an update is found in a dict."""
import functools
from fractions import Fraction

import numpy as np

import trsv_ref as T
from trsv_ref import csr, csr_arrays

RUN, THIN, THIN_MAX = 1024, 256, 1 << 16
LANE_WORK, MAX_BLOCKS = 256, 1024


def constants():
    return dict(ILU0_THIN=THIN, ILU0_THIN_MAX=THIN_MAX, ILU0_MAX_BLOCKS=MAX_BLOCKS, ILU0_FIG_BYTES=16)


def header_footprint(rows, nnz, entries, levels):
    return 4 * (rows + 1) + 20 * rows + 12 * nnz + 16 * entries + 4 * (levels + 1) + 20


# ---- the definition
def slots(mat):
    """-> (cols, a, head): per row the ascending distinct columns inside the matrix, a[r, c] (float64: the entries (r, c) in
    the order given, added left to right from +0.0) and the position of the first entry of every (r, c) group."""
    n, rp, ci, va = mat
    cols, a, head = [], [], []
    for r in range(n):
        acc, first = {}, {}
        for p in range(rp[r], rp[r + 1]):
            c = int(ci[p])
            if 0 <= c < n:
                first.setdefault(c, p)
                acc[c] = acc.get(c, np.float64(0.0)) + np.float64(va[p])
        order = sorted(acc)
        cols.append(order)
        a.append([acc[c] for c in order])
        head.append([first[c] for c in order])
    return cols, a, head


def recurrence(n, cols, a, zero, number):
    """Row-wise IKJ over the slots, in the arithmetic of `number` (np.float64 or Fraction).  -> (w per row, rwork per row);
    a division by an exact zero in fractions raises ZeroDivisionError."""
    w, rwork = [], []
    for r in range(n):
        row = {c: number(v) for c, v in zip(cols[r], a[r])}
        looked = 0
        for k in cols[r]:
            if k >= r:
                break
            piv = w[k].get(k, zero)
            wk = row[k] / piv
            row[k] = wk
            for j in cols[k]:
                if j > k:
                    looked += 1
                    if j in row:
                        p = wk * w[k][j]
                        row[j] = row[j] - p
        w.append(row)
        rwork.append(looked)
    return w, rwork


def factor(mat, f32=1):
    """-> dict(lu, lu64, level, lstart, rwork, entries, levels, max_list, max_width, missing_diag, first_missing, work,
    zero_pivots, first_zero)."""
    n, rp, ci, va = mat
    cols, a, head = slots(mat)
    with np.errstate(all="ignore"):
        w, rwork = recurrence(n, cols, a, np.float64(0.0), np.float64)
    lu64 = np.zeros(len(ci), np.float64)
    level = np.zeros(n, np.int64)
    missing, zero = [], []
    for r in range(n):
        for c, p in zip(cols[r], head[r]):
            lu64[p] = w[r][c]
        lower = [c for c in cols[r] if c < r]
        level[r] = max(level[c] for c in lower) + 1 if lower else 0
        if r not in w[r]:
            missing.append(r)
        if w[r].get(r, np.float64(0.0)) == 0.0:
            zero.append(r)
    levels = int(level.max()) + 1 if n else 0
    width = np.bincount(level, minlength=levels) if n else np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        lu = lu64.astype(np.float32) if f32 else lu64
    return dict(lu=lu, lu64=lu64, level=level.astype(np.int32), lstart=np.concatenate(([0], np.cumsum(width))).astype(np.int64),
                rwork=np.array(rwork, np.int64), entries=sum(len(c) for c in cols), levels=levels,
                max_list=max((len(c) for c in cols), default=0), max_width=int(width.max()) if n else 0,
                missing_diag=len(missing), first_missing=missing[0] if missing else -1, work=int(sum(rwork)),
                zero_pivots=len(zero), first_zero=zero[0] if zero else -1)


def plan(lstart, thin=None, entries=1, nnz=1):
    """-> (launches, runs, levels_in_runs) of a call: ilu0_load where there is a slot, sh_trsv's plan of the levels cut at
    RUN, ilu0_store; nothing for a matrix without rows or without entries."""
    if len(lstart) <= 1 or nnz == 0:
        return 0, 0, 0
    launches, runs, in_runs = T.plan(lstart, thin, RUN)
    return launches + (1 if entries else 0) + 1, runs, in_runs


# ---- exactly, for the small cases
def exact_factor(mat):
    """{(r, c): Fraction} over the slots: the same recurrence without rounding (a[r, c] = the exact sum of the entries)."""
    n = mat[0]
    cols, a, _ = slots(mat)
    exact_a = [[Fraction(0)] * len(c) for c in cols]
    _, rp, ci, va = mat
    for r in range(n):
        at = {c: i for i, c in enumerate(cols[r])}
        for p in range(rp[r], rp[r + 1]):
            if 0 <= ci[p] < n:
                exact_a[r][at[int(ci[p])]] += Fraction(float(va[p]))
    w, _ = recurrence(n, cols, exact_a, Fraction(0), Fraction)
    return {(r, c): v for r in range(n) for c, v in w[r].items()}, {(r, c): v for r in range(n) for c, v in zip(cols[r], exact_a[r])}


def product(n, w):
    """(L U)[i, j] for every (i, j) where it is not zero or is a slot, from the factor's slots: L unit lower, U upper."""
    by_row, out = {}, {}
    for (r, c), v in w.items():
        by_row.setdefault(r, {})[c] = v
    for i in range(n):
        acc = {}
        lrow = {k: v for k, v in by_row.get(i, {}).items() if k < i}   # row i of L: l[i, k] for k < i, and 1 at k = i
        lrow[i] = Fraction(1)
        for k, lik in lrow.items():
            for j, ukj in by_row.get(k, {}).items():
                if j >= k:
                    acc[j] = acc.get(j, Fraction(0)) + lik * ukj
        for j, v in acc.items():
            out[(i, j)] = v
    return out


# ---- the cases: name -> (n, row_ptr, col_idx, val)
def _rng(seed):
    return np.random.default_rng(seed)


def _vals(rng, k, scale=1.0):
    """Drawn non-integer float32 values away from zero, both signs."""
    return (rng.uniform(0.25, 1.75, k) * rng.choice([-1.0, 1.0], k) * scale).astype(np.float32)


def from_dense(a, pattern):
    """CSR of the dense integer matrix `a` on the positions where `pattern` is set (zeros there are stored), the rows
    unsorted (a drawn order)."""
    n = a.shape[0]
    rng = _rng(n)
    ent = []
    for r in range(n):
        cs = np.nonzero(pattern[r])[0]
        for c in rng.permutation(cs):
            ent.append((r, int(c), float(a[r, c])))
    return csr(n, ent)


def exact_pair(kind):
    """(L0, U0): unit lower and upper integer matrices whose product has no fill outside their joint pattern; U0's
    diagonal is drawn from +-1, +-2, +-4."""
    rng = _rng({"dense12": 61, "dense40": 62, "tri30": 63, "arrow": 64}[kind])
    n = {"dense12": 12, "dense40": 40, "tri30": 30, "arrow": 70}[kind]
    i, j = np.indices((n, n))
    if kind.startswith("dense"):
        lo, up = i > j, i < j
    elif kind == "tri30":
        lo, up = i == j + 1, j == i + 1
    else:   # the downward arrow: the last row, the last column and the diagonal
        lo, up = (i == n - 1) & (j < i), (j == n - 1) & (i < j)
    small = lambda: rng.integers(-2, 3, (n, n)).astype(np.float64)   # noqa: E731
    L0 = np.where(lo, small(), 0.0) + np.eye(n)
    U0 = np.where(up, small(), 0.0) + np.diag(rng.choice([1.0, -1.0, 2.0, -2.0, 4.0, -4.0], n))
    return L0, U0, lo | up | (i == j)


@functools.lru_cache(maxsize=None)
def exact_case(kind):
    L0, U0, pattern = exact_pair(kind)
    a = L0 @ U0
    assert np.all(a[~pattern] == 0.0)   # no fill
    return from_dense(a, pattern), L0, U0


def grid_matrix(side=12):
    return T.grid_lower(side)


def drawn_matrix(n=40, per_row=4, seed=65):
    """A drawn pattern with a dominant diagonal: per_row drawn off-diagonal columns per row, not symmetric, rows unsorted."""
    rng = _rng(seed)
    ent = []
    for r in range(n):
        cs = [int(c) for c in rng.choice(n, per_row, replace=False) if c != r]
        vs = _vals(rng, len(cs))
        row = [(r, c, float(v)) for c, v in zip(cs, vs)] + [(r, r, float(np.abs(vs).sum() + rng.uniform(1.0, 2.0)))]
        for i in rng.permutation(len(row)):
            ent.append(row[i])
    return csr(n, ent)


def tiers_matrix():
    """Row 0's column is a hub: every row has the slot (r, 0).  Rows 1 ... 129 are the rows k: 1, 2, 3 and 4 have 63, 64, 65
    and 130 upper slots, the others 2, row 0 has 1.  Row 300 has the 130 lower slots 0 ... 129 (the wave tier; the upper
    slots of rows 1 ... 4 lie among its lower slots: a step's stores are the next steps' loads); rows 350, 351 and 352 sum
    to a share of work of LANE_WORK - 1, LANE_WORK and LANE_WORK + 1."""
    n, R = 400, 300
    rng = _rng(66)
    upper = {0: [R], 1: list(range(2, 65)), 2: list(range(3, 67)), 3: list(range(4, 69)), 4: list(range(5, 135))}
    for k in range(5, 130):
        upper[k] = [R, 301 + k % 40]
    lower = {r: [0] for r in range(1, n)}
    lower[R] = list(range(130))
    lower[350] = [0, 4, 2] + list(range(5, 35))      # 1 + 130 + 64 + 30 * 2
    lower[351] = [0, 4, 3] + list(range(5, 35))      # 1 + 130 + 65 + 30 * 2
    lower[352] = [0, 1, 2, 3] + list(range(5, 37))   # 1 + 63 + 64 + 65 + 32 * 2
    ent = []
    for r in range(n):
        cs = sorted(set(lower.get(r, [])) | set(upper.get(r, [])) | ({R + 1, 399} if r in (R, 350, 351, 352) and r < 399 else set()))
        cs = [c for c in cs if c != r]
        vs = _vals(rng, len(cs), 0.125)
        row = [(r, c, float(v)) for c, v in zip(cs, vs)] + [(r, r, float(rng.uniform(8.0, 9.0)))]
        for i in rng.permutation(len(row)):
            ent.append(row[i])
    return csr(n, ent)


def path_matrix(n):
    """Tridiagonal with a dominant diagonal: `n` levels of one row."""
    rng = _rng(67)
    r = np.concatenate([np.arange(n), np.arange(1, n), np.arange(n - 1)])
    c = np.concatenate([np.arange(n), np.arange(n - 1), np.arange(1, n)])
    v = np.concatenate([rng.uniform(4.0, 5.0, n), _vals(rng, 2 * (n - 1))])
    return csr_arrays(n, r, c, v)


def widths_matrix(t):
    """Consecutive levels of t - 1, t, t + 1, 1 and t + 1 rows: every row of a level has two drawn lower slots in the level
    before, and the pattern is symmetric (the upper slots are what the next level's rows subtract)."""
    rng = _rng(68 + t)
    widths = [t - 1, t, t + 1, 1, t + 1]
    start = np.concatenate(([0], np.cumsum(widths)))
    n = int(start[-1])
    r, c = [], []
    for L in range(1, len(widths)):
        rows = np.arange(start[L], start[L + 1])
        for _ in range(2):
            r.append(rows)
            c.append(rng.integers(start[L - 1], start[L], len(rows)))
    r, c = np.concatenate(r), np.concatenate(c)
    pairs = np.unique(np.stack([np.concatenate([r, c]), np.concatenate([c, r])]), axis=1)
    k = pairs.shape[1]
    return csr_arrays(n, np.concatenate([np.arange(n), pairs[0]]), np.concatenate([np.arange(n), pairs[1]]),
                      np.concatenate([rng.uniform(8.0, 9.0, n), _vals(rng, k)]))


def wide_matrix():
    """A diagonal plus one dense column: level 1 holds more rows than a capped launch has lanes (MAX_BLOCKS * 256); row 0
    has five upper slots, so every row looks five columns up (and rows 1 ... 5 find their diagonal)."""
    rng = _rng(69)
    n = MAX_BLOCKS * 256 + 5
    r = np.concatenate([np.arange(n), np.arange(1, n), np.zeros(5, np.int64)])
    c = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64), np.arange(1, 6)])
    v = np.concatenate([rng.uniform(4.0, 5.0, n), _vals(rng, n - 1), _vals(rng, 5)])
    return csr_arrays(n, r, c, v)


GUARD = 1.0e30   # a value that would change the factor visibly if an ignored entry were read


def dirt_matrix():
    """Unsorted rows, parallel entries (a doubled diagonal too), columns -1 and rows with guard values, a missing diagonal
    (row 5), [[1, 1], [1, 1]] in rows 6 and 7 (row 7's pivot becomes zero), explicit zeros, -0.0, inf and NaN values."""
    n = 14
    ent = [
        (0, 0, 2.0), (0, 3, 0.5), (0, -1, GUARD), (0, n, GUARD), (0, 1, -0.25),
        (1, 1, 0.75), (1, 0, 0.5), (1, 1, 0.5), (1, 0, -0.125), (1, 2, 0.3),          # doubled diagonal, parallel (1, 0)
        (2, 1, 0.3), (2, 2, 1.1), (2, 0, -0.7), (2, 1, 0.9), (2, 0, 0.2), (2, 3, 0.1),   # unsorted, parallel
        (3, 3, 3.0), (3, 0, 0.0), (3, 2, -0.0), (3, 4, 1.0),                          # explicit zeros
        (4, 2, 1.25), (4, 4, -1.5), (4, 2 ** 31 - 1, GUARD), (4, -2 ** 31, GUARD), (4, 5, 0.5),
        (5, 1, 0.6), (5, 4, -0.4), (5, 6, 0.7),                                       # no diagonal
        (6, 6, 1.0), (6, 7, 1.0),
        (7, 6, 1.0), (7, 7, 1.0), (7, 8, 2.0),                                        # 1 - 1 * 1: a zero pivot
        (8, 7, 3.0), (8, 8, 1.0), (8, 5, 0.5),                                        # divides by it: inf, and by row 5's +0.0
        (9, 9, -0.0), (9, 10, 1.0),                                                   # a pivot of -0.0 counts
        (10, 9, 0.0), (10, 10, 2.0),                                                  # 0 / -0.0: NaN
        (11, 11, np.inf), (11, 12, 1.0), (11, 0, 1.0),
        (12, 11, 1.0), (12, 12, np.nan), (12, 13, -0.0),                              # a NaN pivot does not count
        (13, 12, 1.0), (13, 13, 1.0), (13, 3, -0.0),
    ]
    return csr(n, ent)


CASES = {
    "exact-dense12": lambda: exact_case("dense12")[0],
    "exact-dense40": lambda: exact_case("dense40")[0],
    "exact-tri30": lambda: exact_case("tri30")[0],
    "exact-arrow": lambda: exact_case("arrow")[0],
    "grid12": lambda: grid_matrix(12),
    "drawn40": lambda: drawn_matrix(),
    "tiers": tiers_matrix,
    "path-runs": lambda: path_matrix(2 * RUN + 3),
    "widths64": lambda: widths_matrix(64),
    "widths256": lambda: widths_matrix(THIN),
    "wide": wide_matrix,
    "dirt": dirt_matrix,
    "rows0": lambda: csr(0, []),
    "rows1": lambda: csr(1, [(0, 0, 2.5)]),
    "rows1-empty": lambda: csr(1, []),
    "nnz0": lambda: csr(5, []),
}
EXACT = ("exact-dense12", "exact-dense40", "exact-tri30", "exact-arrow")
ROUNDED = ("grid12", "drawn40")   # the cases the distance from the fractions is measured on
NOTHING = ("rows0", "rows1-empty", "nnz0")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def want(name, f32=1):
    """factor(case(name), f32), the recurrence run once per case."""
    if f32:
        w = dict(want(name, 0))
        with np.errstate(all="ignore"):
            w["lu"] = w["lu64"].astype(np.float32)   # each rounded once on the way out
        return w
    return factor(case(name), 0)


def same_bits(a, b):
    """== on bit patterns, a NaN standing where a NaN stands."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
