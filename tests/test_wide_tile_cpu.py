"""The WIDE x tile of the tiled plan, without a GPU: the host builder (plan_host.h) and the host emulation of both
phases (debug_tools.h) through the tools build, with the wide layout forced by SH_TILE_COLS=wide.  A wide layout's
column codes use all 16 bits and its fold flags live in fmask[], one 64-bit word per block of obase[]; what is checked
here is that no column code at or above 32 768 is ever read as a flag, that the masks say what the narrow builder's
flags say, that two-byte codes keep the narrow tile, and that nothing moves for a matrix that does not get the wide
tile.  Weights and x are small integers: every sum is exact in float32 and results are compared for equal bits."""
import ctypes as C

import numpy as np
import pytest

from sparseharness_amd import abi
from test_plan_cpu import _p, emu, emulate, exact, random_matrix   # noqa: F401  (emu: the fixture that builds and loads emulate.so)

NARROW = 32760


@pytest.fixture()
def lay(emu):
    emu.sh_debug_plan_layout.restype = C.c_int
    emu.sh_debug_plan_layout.argtypes = ([C.c_int64] * 3 + [C.c_void_p] * 3 + [C.POINTER(abi.sh_plan_options), C.c_int, C.c_void_p] +
                                         [C.c_void_p, C.c_int64] * 4)
    return emu


def layout(lib, rows, cols, rp, ci, va, **options):
    """The host-built layout: its numbers, first column codes, obase, fmask and describe string (None: refused)."""
    opt = abi.sh_plan_options()
    lib.sh_plan_options_default(C.byref(opt))
    opt.plan = 2
    for k, v in options.items():
        setattr(opt, k, v)
    info = np.zeros(10, np.int64)
    args = [rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), 256]
    text = C.create_string_buffer(512)
    if lib.sh_debug_plan_layout(*args, _p(info), None, 0, None, 0, None, 0, text, 512) != 0:
        return None
    tcol, obase, fmask = np.zeros(max(int(info[2]), 1), np.uint16), np.zeros(int(info[6]), np.uint32), np.zeros(max(int(info[7]), 1), np.uint64)
    assert lib.sh_debug_plan_layout(*args, _p(info), _p(tcol), len(tcol), _p(obase), len(obase), _p(fmask), int(info[7]), None, 0) == 0
    names = ("tcols", "tiles", "stream", "light_len", "products", "code_bits", "obase_words", "fmask_words", "items", "hash")
    return dict(zip(names, info.tolist()), tcol=tcol[:int(info[2])], obase=obase, fmask=fmask[:int(info[7])], describe=text.value.decode())


@pytest.fixture()
def wide(monkeypatch):
    monkeypatch.setenv("SH_TILE_COLS", "wide")


@pytest.fixture()
def W(lay, wide):
    """The wide width, as a layout reports it."""
    rp, ci, va = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1], np.float32)
    w = layout(lay, 1, 5, rp, ci, va)["tcols"]
    assert 32768 < w <= 65528 and w % 8 == 0
    return w


def pack_products(np_, ns):
    """plan_common.h::pack_piece: the products of a (bin, tile) piece with np_ pairs and ns singles."""
    blocks = (np_ + 3) // 4
    sg = (max(ns - (4 * blocks - np_), 0) + 3) // 4
    if blocks > 0 and sg == 0:
        sg = 1
    return 4 * (blocks + sg)


def csr(rows_cols):
    rp = np.zeros(len(rows_cols) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows_cols])
    ci = np.array([c for r in rows_cols for c in r], np.int32)
    va = (1 + np.arange(len(ci)) % 5).astype(np.float32)
    return rp, ci, va


def check(lib, rows, cols, rp, ci, va, **options):
    rc, y, st, x = emulate(lib, rows, cols, rp, ci, va, 0, **options)
    assert rc == 0 and st["poison_reads"] == 0, (rc, st)
    np.testing.assert_array_equal(y, exact(rows, cols, rp, ci, va, x, 0))
    return st


def test_bit_15_of_a_column_code_is_a_column_bit(lay, W):
    cols = W + 8
    # row 0: ONE entry at 32 768, the first single of tile 0 -- the first code of a singles group; rows 1..8: two entries
    # each, both at or above 32 768 and in tile 0: eight pairs = two full pair blocks; then the columns on both sides of
    # bit 15 and of the tile seam
    rows_cols = [[32768]] + [[32768 + 3 * k, W - 2 - 5 * k] for k in range(1, 9)] + [[0], [32767], [W - 1], [W], [W + 7]]
    rp, ci, va = csr(rows_cols)
    rows = len(rows_cols)
    st = check(lay, rows, cols, rp, ci, va)
    L = layout(lay, rows, cols, rp, ci, va)
    assert (L["tcols"], L["tiles"]) == (W, 2) and f" tile={W}" in L["describe"]
    # tile 0: 8 pairs + 4 singles, tile 1: 2 singles; unfolded: 20 and 2 singles
    assert st["products"] == L["products"] == pack_products(8, 4) + pack_products(0, 2) == 16
    assert check(lay, rows, cols, rp, ci, va, fold=0)["products"] == pack_products(0, 20) + pack_products(0, 2) == 24
    # the single at 32 768 leads a group, and that group does not fold; the groups that do are the B groups of the pair blocks
    first = L["tcol"][: L["light_len"] : 4]
    bits = np.array([(int(L["fmask"][g // 64]) >> (g % 64)) & 1 for g in range(len(first))])
    lead = np.flatnonzero(first == 32768)
    assert len(lead) == 1 and bits[lead[0]] == 0
    assert bits.sum() == 2 and (np.flatnonzero(bits) % 2 == 1).all()
    assert (L["tcol"] >= 32768).sum() >= 17 and L["tcol"].max() == W      # codes with bit 15 set; the identity code is W


@pytest.mark.parametrize("short", [0, 3])
def test_one_tile_full_and_partial(lay, W, short):
    cols = W - short
    rng = np.random.default_rng(7 + short)
    rp, ci, va = random_matrix(rng, 600, cols, 9, 2, hlen=1500)
    ci[:4] = [0, cols - 1, 32768, 32767]
    st = check(lay, 600, cols, rp, ci, va)
    assert st["tiles"] == 1 and st["heavy_rows"] >= 1
    assert layout(lay, 600, cols, rp, ci, va)["tcol"].max() == W            # padding reads the slot behind the tile


def test_fold_masks_are_the_narrow_builders_flags(lay, monkeypatch):
    """One tile in both layouts (every column below 32 760), pieces of ~200 groups whose pairs cross the 64-group blocks,
    a last block that is partial: bit i of a block's mask = bit 15 of the first code of its group i in the narrow layout."""
    rng = np.random.default_rng(11)
    rows = 5000
    rows_cols = [sorted(rng.choice(NARROW, int(d), replace=False).tolist()) for d in rng.integers(0, 5, rows)]
    rp, ci, va = csr(rows_cols)
    monkeypatch.setenv("SH_TILE_COLS", "narrow")
    N = layout(lay, rows, NARROW, rp, ci, va)
    monkeypatch.setenv("SH_TILE_COLS", "wide")
    Wd = layout(lay, rows, NARROW, rp, ci, va)
    check(lay, rows, NARROW, rp, ci, va)
    assert N["tcols"] == NARROW and N["fmask_words"] == 0 and Wd["tcols"] > NARROW
    assert (N["tiles"], N["stream"], N["products"]) == (Wd["tiles"], Wd["stream"], Wd["products"]) == (1, N["stream"], N["products"])
    np.testing.assert_array_equal(N["obase"], Wd["obase"])
    groups = N["light_len"] // 4
    assert groups > 64 * 3 and Wd["fmask_words"] == Wd["obase_words"] == groups // 64 + 1
    assert N["tcol"][N["light_len"] - 4] == NARROW and N["tcol"][N["light_len"] - 256] != NARROW   # the last block is partial
    flags = (N["tcol"][: N["light_len"] : 4] >> 15).astype(np.uint64)
    want = np.zeros(Wd["fmask_words"], np.uint64)
    for g in np.flatnonzero(flags):
        want[g // 64] |= np.uint64(1) << np.uint64(g % 64)
    assert flags.sum() > 500
    np.testing.assert_array_equal(Wd["fmask"], want)
    assert any(int(m) >> 63 for m in want) and any(int(m) & 2 for m in want)   # flags in the last and the second lane of a block
    # the column codes are the same but for the flag bit and the identity code
    nt, wt = N["tcol"].astype(np.int64) & 0x7FFF, Wd["tcol"].astype(np.int64)
    np.testing.assert_array_equal(np.where(nt == NARROW, -1, nt), np.where(wt == Wd["tcols"], -1, wt))


def test_two_byte_codes_keep_the_narrow_tile(lay, W):
    rng = np.random.default_rng(13)
    rows, cols = 2000, W + 500
    rp, ci, va = random_matrix(rng, rows, cols, 10, 1)
    va = (1 + np.arange(len(va)) % 700).astype(np.float32)                   # 700 distinct words: two-byte codes
    L = layout(lay, rows, cols, rp, ci, va)
    assert (L["code_bits"], L["tcols"], L["fmask_words"]) == (16, NARROW, 0) and "tile=" not in L["describe"]
    assert L["tiles"] == -(-cols // NARROW)
    x = (1 + np.arange(cols) % 3).astype(np.float32)                          # sums below 2^24
    rc, y, st, _ = emulate(lay, rows, cols, rp, ci, va, 0, x=x)
    assert rc == 0 and st["poison_reads"] == 0
    np.testing.assert_array_equal(y, exact(rows, cols, rp, ci, va, x, 0))
    # ... and the same matrix with few values goes wide under the same override
    assert layout(lay, rows, cols, rp, ci, np.minimum(va, 9))["tcols"] == W


@pytest.mark.parametrize("coding", [0, 8, -1])
def test_below_the_threshold_the_default_is_the_narrow_layout(lay, monkeypatch, coding):
    rng = np.random.default_rng(17)
    rows, cols = 3000, 100_000
    rp, ci, va = random_matrix(rng, rows, cols, 12, 3)
    monkeypatch.delenv("SH_TILE_COLS", raising=False)
    D = layout(lay, rows, cols, rp, ci, va, value_coding=coding)
    monkeypatch.setenv("SH_TILE_COLS", "narrow")
    N = layout(lay, rows, cols, rp, ci, va, value_coding=coding)
    assert D["describe"] == N["describe"] and "tile=" not in D["describe"] and D["hash"] == N["hash"]
    assert D["tcols"] == NARROW and D["tiles"] == 4 and D["fmask_words"] == 0
    np.testing.assert_array_equal(D["tcol"], N["tcol"])
    np.testing.assert_array_equal(D["obase"], N["obase"])
    monkeypatch.setenv("SH_TILE_COLS", "wide")
    assert layout(lay, rows, cols, rp, ci, va, value_coding=coding)["hash"] != N["hash"]
