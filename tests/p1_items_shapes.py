"""Matrices for the tests of the phase-1 work items (tests/test_p1_items_cpu.py, tests/test_p1_items_gpu.py).

A column tile holds 32 768 columns; a row is heavy from max(512, 8 * tiles) entries on; a heavy run is cut at multiples
of 1024 entries (64 strips of 16); small matrices get items of 48 K entries.  Weights are 1..16 and x is 1 + c % 3, so a
row of up to 349 K entries sums exactly in float32 in any order (349 525 * 48 < 2^24): every path gives the same bits."""
import numpy as np

TCOLS = 32768
WAVE = 64 * 16   # entries of one wave of heavy strips

# name: rows, columns, mean light degree, heavy rows, entries per heavy row
SHAPES = {
    "one_tile": (4000, 30_000, 10, 2, 120_000),                 # one heavy run of 240 K entries: five items
    "nine_tiles_three_heavy": (20_000, 9 * TCOLS, 10, 3, 300_000),   # 100 K heavy entries per tile: three items each
    "short_heavy_run": (3000, 2 * TCOLS, 8, 1, 700),            # 350 heavy entries per tile: less than one strip-wave
    "eighth_shard": (30_000, 39 * TCOLS, 12, 4, 200_000),       # 39 tiles as an eighth of the headline matrix: ~80 items
}


def matrix(name):
    rows, cols, avg, heavy, hlen = SHAPES[name]
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 900)
    deg = rng.poisson(avg, rows).astype(np.int64)
    deg[rng.integers(0, rows, rows // 10)] = 0
    deg[rng.choice(rows, heavy, replace=False)] = hlen
    rp = np.zeros(rows + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    va = rng.integers(1, 17, nnz).astype(np.float32)
    return rows, cols, rp, ci, va


def x_float(cols):
    return (1 + np.arange(cols) % 3).astype(np.float32)
