"""Patterns of the square test matrices that tests/test_frontier_gpu.py, tests/test_bfs_levels_gpu.py and
tests/test_sssp_gpu.py share.  Each of those files puts values of its own on them."""
import numpy as np


def rows_of_entries(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int32), np.diff(rp))


def ragged_pattern(seed=77, n=3001, long_len=20_001):
    """-> (rng, row_ptr, col_idx).  Like ragged_csr of tests/test_bits_gpu.py, but square: empty rows, short and medium
    rows, ONE row of 20 001 entries (above the long-row threshold), ONE column of 20 001 entries (spread over all rows,
    several per row), column indices outside [0, n) on both sides.  The generator comes back in the state the pattern
    left it in: the caller draws its values from it."""
    rng = np.random.default_rng(seed)
    hub = 7
    deg = rng.integers(0, 12, n)
    deg[rng.random(n) < 0.3] = 0
    deg[rng.integers(0, n, 40)] = rng.integers(17, 300, 40)
    deg[n // 3] = long_len
    deg[0] = 3
    deg[n - 1] = 5
    extra = np.full(n, long_len // n, np.int64)   # entries of the hub column per row
    extra[: long_len - extra.sum()] += 1
    extra[rng.random(n) < 0.2] = 0                # (some rows stay empty) ...
    extra[n // 2] += long_len - extra.sum()       # ... and one row makes the count up
    tot = deg + extra
    rp = np.concatenate([[0], np.cumsum(tot)]).astype(np.int32)
    ci = rng.integers(0, n, rp[-1]).astype(np.int32)
    ci[ci == hub] = hub + 1
    oob = rng.random(rp[-1]) < 0.03
    ci[oob] = np.where(rng.random(oob.sum()) < 0.5, -1 - rng.integers(0, 5, oob.sum()), n + rng.integers(0, 1000, oob.sum()))
    for r in range(n):                            # the hub entries sit at the end of each row
        ci[rp[r + 1] - extra[r]: rp[r + 1]] = hub
    assert (ci == hub).sum() == long_len and tot[n // 3] >= long_len and (tot == 0).any()
    return rng, rp, ci


# List lengths that sit on the thresholds of the worklist kernels: one lane per list up to 8 (32 in the bottom-up BFS),
# the whole wave up to a piece (64 entries per wave step), pieces of 2048 (out-lists, columns) and 4096 (rows); 8192 is
# exactly two pieces of 4096 and four of 2048.
EDGE_LENGTHS = (1, 8, 9, 32, 33, 64, 65, 2048, 2049, 4096, 4097, 8192)
EDGE_N = 16_384
EDGE_SOURCES = (0, 8192)


def edges_pattern():
    """-> (row_ptr, col_idx) of "edges": vertex 8192 + k has an entry in columns 0 .. L - 1 for the k-th L of
    EDGE_LENGTHS, plus the transpose of all that.  So vertex 8192 + k has a row and a column of exactly L entries, the
    vertices below 8192 have rows of up to 12, the matrix is symmetric, everything is within three hops of vertex
    8192 + 11, and the rest of the upper half has empty rows."""
    hubs = np.concatenate([np.full(L, 8192 + k, np.int64) for k, L in enumerate(EDGE_LENGTHS)])
    low = np.concatenate([np.arange(L, dtype=np.int64) for L in EDGE_LENGTHS])
    rows, cols = np.concatenate([hubs, low]), np.concatenate([low, hubs])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=EDGE_N))]).astype(np.int32)
    return rp, cols[order].astype(np.int32)


def assert_edge_lengths(rp, ci):
    """Every length of EDGE_LENGTHS occurs as a row's and as a column's."""
    by_row, by_col = np.bincount(rows_of_entries(rp), minlength=EDGE_N), np.bincount(ci, minlength=EDGE_N)
    assert set(EDGE_LENGTHS) <= set(by_row.tolist()) and set(EDGE_LENGTHS) <= set(by_col.tolist())
    assert len(rp) - 1 == EDGE_N and by_row[: 8192].max() == len(EDGE_LENGTHS) and not by_row[8192 + len(EDGE_LENGTHS):].any()


def sources(name):
    """The source vertices a traversal test starts from, one run each."""
    return EDGE_SOURCES if name == "edges" else (0,)
