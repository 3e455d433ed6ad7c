"""Small matrices that reach the refusal rules of the x-tiled layout ("Limits of the tiled layout"), shared
by tests/test_plan_limits_cpu.py (host builder, through the emulator) and tests/test_plan_limits_gpu.py (both builders,
and the upload).  All deterministic, all with small integer values, so that every (+,x) sum is exact in any order.

The numbers of the layout the arithmetic below relies on (kernels.hip.h): a column tile has TCOLS = 32760 columns, a row
bin at most TBIN_ROWS = 2048 rows, a light (bin, tile) piece is padded to whole groups of 4 stream entries, a tile's light
run to 256 entries, a heavy (row, tile) piece to whole strips of 16, and a row is heavy from max(512, 8 * tiles) entries.
A layout is refused when its stream is longer than nnz + nnz / 4 + 4096 + 256 * tiles entries."""
import numpy as np

TCOLS, TBIN_ROWS = 32760, 2048
TILES = 62
COLS = TILES * TCOLS

WHY_PADDING = "padding would cost more than 25 %"
WHY_TILES = "not applicable"
WHY_P = "P exceeds 32-bit byte offsets"


def stream_limit(nnz, tiles):
    return nnz + nnz // 4 + 4096 + 256 * tiles


def light_pieces(bins):
    """`bins` row bins of 2048 rows over 62 column tiles, one entry per (bin, tile): row t of a bin holds the bin's entry
    in tile t.  Every entry is a piece of its own, padded to a group of 4, and every tile's run of 4 * bins entries is
    padded to a multiple of 256: stream = 62 * roundup(4 * bins, 256) against stream_limit(62 * bins, 62)."""
    rows = bins * TBIN_ROWS
    deg = np.zeros(rows, np.int64)
    r = (np.arange(bins)[:, None] * TBIN_ROWS + np.arange(TILES)[None, :]).ravel()
    deg[r] = 1
    rp = np.zeros(rows + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    k = np.arange(bins * TILES)
    ci = ((k % TILES) * TCOLS + (k * 37) % TCOLS).astype(np.int32)
    va = (1 + k % 5).astype(np.float32)
    return rows, COLS, rp, ci, va


def light_stream_len(bins):
    return TILES * ((4 * bins + 255) // 256 * 256)


def heavy_strips(nrows):
    """`nrows` rows of 512 entries, entry k of a row in tile k % 62: heavy rows (512 >= max(512, 8 * 62)), 8 or 9 entries
    per (row, tile) piece, each padded to a strip of 16: stream = 992 * nrows against stream_limit(512 * nrows, 62) =
    640 * nrows + 19968.  The verdict flips between 56 rows (55552 <= 55808) and 57 rows (56544 > 56448), which pins the
    rule's quarter within about a percent and its constant within 256 entries."""
    per = 512
    rp = (np.arange(nrows + 1) * per).astype(np.int32)
    k = np.arange(nrows * per)
    row, j = k // per, k % per
    ci = ((j % TILES) * TCOLS + (row * 101 + (j // TILES) * 613) % TCOLS).astype(np.int32)
    va = (1 + (k % 7)).astype(np.float32)
    return nrows, COLS, rp, ci, va


def heavy_stream_len(nrows):
    return 992 * nrows


def too_many_tiles():
    """One row, two entries, 2^31 - 1 columns: 65553 column tiles, more than the 65535 a 16-bit tile number names."""
    cols = 2 ** 31 - 1
    rp = np.array([0, 2], np.int32)
    ci = np.array([5, cols - 1], np.int32)
    va = np.array([1, 2], np.float32)
    return 1, cols, rp, ci, va


# the table of the layout's limits that small matrices reach: name -> (matrix, built?, the device builder's reason)
TABLE = {
    "light_150_bins": (lambda: light_pieces(150), False, WHY_PADDING),
    "light_60_bins": (lambda: light_pieces(60), True, ""),
    "light_64_bins": (lambda: light_pieces(64), True, ""),      # 62 * 256 = 15872 <= 24928
    "light_65_bins": (lambda: light_pieces(65), False, WHY_PADDING),   # 62 * 512 = 31744 > 25005: the run's padding to 256 tips it
    "heavy_100_rows": (lambda: heavy_strips(100), False, WHY_PADDING),
    "heavy_56_rows": (lambda: heavy_strips(56), True, ""),
    "heavy_57_rows": (lambda: heavy_strips(57), False, WHY_PADDING),
    "tiles_65553": (too_many_tiles, False, WHY_TILES),
}
