"""The inputs of tests/test_hygiene_gpu.py, proven on the CPU from the references alone (tests/hygiene_shapes.py):
  - a poison word that reaches a row's reduction changes that row's output word: for every row under (+,x), (min,+) and
    (max,min); under (or,and) for at least half of the non-empty light rows, for both heavy rows of the tiled shapes
    and, under the all-zero x, for the long rows of the stream shape;
  - the liveness patterns are what they claim, tile by tile;
  - the tiled shapes have the tiles, row bins and heavy rows that reach every scratch array, and the layout walked on
    the host (sh_debug_emulate_plan) reads no product that it did not write and gives the oracle's row sums;
  - each value set selects the phase-1 instantiation it is named after;
  - the same for every rotated (x, y) pair that the multi-vector launches use;
  - every loop of the path-with-chords graph needs more than one batch of eight launches, the loop on the stream
    shape reaches its long row, and the three-tile path is live in every tile of every launch."""
import ctypes as C

import numpy as np
import pytest

import hygiene_shapes as S
from oracle import oracle as O
from sparseharness_amd import abi
from test_plan_cpu import _p, emu, emulate  # noqa: F401  (emu: the fixture that builds and loads the tools library)

XS = ("A", "B", "0")


def cases():
    for shape in S.SHAPES:
        for vset in (S.VALUE_SETS if shape in S.TILED else ("nibble16",)):
            yield shape, vset


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_a_poison_in_a_row_sum_changes_the_row(sr):
    for shape, vset in cases():
        rows, cols, rp, ci = S.pattern(shape)
        heavy = S.heavy_columns(shape)[0]
        assert len(heavy) == 2 if shape in S.TILED else np.diff(rp)[heavy].max() >= 20_001
        light = np.diff(rp) > 0
        light[heavy] = False
        for which in XS:
            vis = S.visible(sr, shape, vset, which)
            share = float(vis[light].mean())
            print(f"{S.SR_NAME[sr]} {shape} {vset} x_{which}: visible in {int(vis.sum())} of {rows} rows, "
                  f"{share:.3f} of the non-empty light rows, heavy rows {vis[heavy].tolist()}")
            if sr == S.OA:
                assert share >= 0.5, (shape, vset, which, share)
                # (the stream shape's long row reads nearly every column: its result is 0 under x_0 only)
                assert vis[heavy].all() or (shape == "stream" and which != "0"), (shape, vset, which)
            else:
                assert vis.all(), (shape, vset, which, np.nonzero(~vis)[0][:6])


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_a_poison_changes_the_row_in_every_column_of_the_multi_vector_launches(sr):
    """sh_spmm and sh_bits_spmv run on rolled copies of x_A, x_B, x_0 and of y (hygiene_shapes.column_of): the same
    condition for every (x, y) pair that any launch of width 4 or 32, or of 1 or 8 words, uses."""
    rows, cols, rp, ci = S.pattern("stream")
    heavy = S.heavy_columns("stream")[0]
    light = np.diff(rp) > 0
    light[heavy] = False
    shares = []
    for j in range(32):
        for which in XS:                      # column j of launch k holds x of launch k + j: every x meets every j
            x, y = S.rolled_x(sr, which, j), S.y_column_of(sr, j)
            vis, clean = S.visible_xy(sr, "stream", "nibble16", x, y)
            if sr == S.MP:
                assert (S.bits(clean) != 0).all(), (j, which)
            if sr == S.OA:
                shares.append(float(vis[light].mean()))
                assert shares[-1] >= 0.5, (j, which, shares[-1])
                if which == "0":   # the long rows show a poison wherever the epilogue's own y word is 0: the 20 001-entry row in every column of width 4
                    assert np.array_equal(vis[heavy], y[heavy] == 0) and (j >= 4 or vis[np.argmax(np.diff(rp))]), (j, vis[heavy])
            else:
                assert vis.all(), (j, which, np.nonzero(~vis)[0][:6])
    for k in range(len(S.SEQUENCE)):
        for j in (0, 3, 31):
            assert np.array_equal(S.column_of(sr, k, j), S.rolled_x(sr, S.SEQUENCE[(k + j) % 5], j))
    if shares:
        print(f"or_and, rolled columns: visible in {min(shares):.3f} .. {max(shares):.3f} of the non-empty light rows")


def test_no_true_min_plus_word_is_zero():
    """+0.0 is the (min,+) poison and what fresh memory holds: a result that is 0 anyway would hide it."""
    for shape, vset in cases():
        for which in XS:
            assert (S.bits(S.want(S.MP, shape, vset, which)) != 0).all()


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_liveness_patterns(sr, shape):
    rows, cols, rp, ci = S.pattern(shape)
    seg = np.arange(cols) // S.segment_of(shape)
    n_seg = int(seg.max()) + 1
    assert n_seg == (2 if shape == "tiled2" else 3)
    dead = S.bits(np.array([S.ABSORBING[sr]]))[0]
    for which, live_in in (("A", {0, 2}), ("B", {1}), ("0", set())):
        x = S.bits(S.x_vector(sr, shape, which))
        for t in range(n_seg):
            live = bool((x[seg == t] != dead).any())
            assert live == (t in live_in), (which, t)
    if shape in S.TILED:   # the last column is read, and by a live word of x_A or x_B
        assert ci.max() == cols - 1 and ci.min() == 0
        assert cols % 4 == (3 if shape == "tiled3" else 0)


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("vset", sorted(S.VALUE_SETS))
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_tiled_shapes_reach_every_scratch_array(emu, shape, vset, fold):
    rows, cols, rp, ci = S.pattern(shape)
    for sem, sr in ((0, S.PT), (2, S.OA), (3, S.MM)):
        va = S.values_for(sr, shape, vset)
        for which in XS:
            rc, y, st, _ = emulate(emu, rows, cols, rp, ci, va, sem, x=S.x_vector(sr, shape, which), fold=fold)
            assert rc == 0, (rc, st)
            assert st["tiles"] == (3 if shape == "tiled3" else 2) and st["bins"] >= 3 and st["heavy_rows"] == 2, st
            assert st["poison_reads"] == 0, st
            np.testing.assert_array_equal(S.bits(y), S.bits(S.row_sums(sr, shape, vset, which)), err_msg=str((shape, vset, sem, which)))


@pytest.mark.parametrize("vset", sorted(S.VALUE_SETS))
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_each_value_set_selects_its_coding(emu, shape, vset):
    emu.sh_debug_plan_coding.restype = C.c_int
    emu.sh_debug_plan_coding.argtypes = [C.c_int64] * 3 + [C.c_void_p] * 3 + [C.POINTER(abi.sh_plan_options)] + [C.POINTER(C.c_int32)] * 2
    rows, cols, rp, ci = S.pattern(shape)
    distinct, code_bits = S.VALUE_SETS[vset]
    for sr in (S.PT, S.OA):
        va = S.values_for(sr, shape, vset)
        assert len(np.unique(S.bits(va))) == distinct
        opt = abi.sh_plan_options()
        emu.sh_plan_options_default(C.byref(opt))
        opt.plan = 2
        got_bits, got_n = C.c_int32(-1), C.c_int32(-1)
        assert emu.sh_debug_plan_coding(rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), C.byref(got_bits), C.byref(got_n)) == 0
        assert got_bits.value == code_bits, (vset, got_bits.value, got_n.value)
        if code_bits:   # (the padding word 0 takes a code of its own unless exactly 16 values fill the four-bit table)
            assert got_n.value == distinct + (0 if distinct == 16 else 1)


def test_plus_times_sums_are_exact_in_any_order():
    for shape, vset in cases():
        rows, cols, rp, ci = S.pattern(shape)
        va = S.values(shape, vset)
        c = np.clip(ci, 0, cols - 1)
        for which in XS:
            x = S.x_vector(S.PT, shape, which).astype(np.int64)
            total = np.zeros(rows, np.int64)
            np.add.at(total, np.repeat(np.arange(rows), np.diff(rp)), va * x[c])
            assert total.max() < 2 ** 24


def test_stream_shape_has_its_long_row():
    rows, cols, rp, ci = S.pattern("stream")
    assert rows == cols and np.diff(rp).max() >= 20_001 and (ci < 0).any() and (ci >= cols).any()


@pytest.mark.parametrize("sr", (S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_loops_need_more_than_one_batch(sr):
    n, rp, ci = S.loop_graph()
    assert n == 2000 and len(ci) == (n - 1) + (n - S.LOOP_CHORD)
    counts = []
    for v in S.LOOP_SOURCES:
        x, it, conv = S.loop_ref(sr, v)
        assert conv and it < S.LOOP_CAP
        counts.append(it)
    print(f"{S.SR_NAME[sr]}: launches per source {counts}")
    assert max(counts) > 8 and counts[0] > 16
    if sr == S.OA:
        for v in S.LOOP_SOURCES:
            sizes = S.loop_levels(v)
            assert len(sizes) == S.loop_ref(sr, v)[1] and sizes[-1] == 0
            assert sum(sizes) + 1 == int((S.loop_ref(sr, v)[0] != 0).sum())


@pytest.mark.parametrize("sr", (S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_the_stream_shape_iterates_across_a_batch_seam_or_near_it(sr):
    va, x0, x, it, conv = S.stream_loop(sr)
    print(f"{S.SR_NAME[sr]}: {it} launches on the stream shape")
    assert conv and 3 <= it < S.STREAM_CAP
    assert (S.bits(x) != S.bits(x0)).sum() > 1000      # the source reaches most of the graph, the long row included
    rows, cols, rp, ci = S.pattern("stream")
    long_row = int(np.argmax(np.diff(rp)))
    assert S.bits(x)[long_row] != S.bits(x0)[long_row]


@pytest.mark.parametrize("sr", (S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_every_tile_of_the_long_path_is_live_in_every_launch(sr):
    """The input of each of the 20 launches holds, in each of the three column tiles, words that are not the
    background (nor the absorbing word), and in tiles 0 and 1 more of them than in the launch before: a wrong or
    shifted staging of any tile changes output words."""
    n, rp, ci = S.long_path()
    va, x0 = S.long_case(sr)
    assert n == 2 * S.TCOLS + 3 and n % 4 == 3
    tile = np.arange(n) // S.TCOLS
    bg = S.bits(np.array([S.LONG_BACKGROUND[sr]], O.elem_dtype(sr)))[0]
    dead = S.bits(np.array([S.ABSORBING[sr]]))[0]
    x, before = x0, None
    for launch in range(S.LONG_CAP):
        w = S.bits(x)
        counts = [int(((w[tile == t] != bg) & (w[tile == t] != dead)).sum()) for t in range(3)]
        assert min(counts) >= 1, (launch, counts)
        if before is not None:
            assert counts[0] > before[0] and counts[1] > before[1], (launch, before, counts)
        before = counts
        x = O.kernel(sr, rp, ci, va, x, x0, *S.LOOP_SCALARS[sr])
    want, it, conv = S.long_ref(sr)
    assert (it, conv) == (S.LONG_CAP, False) and np.array_equal(S.bits(x), S.bits(want))
    assert S.bits(want)[n - 1] != bg and S.bits(want)[n - 2] != bg     # the last tile's three columns carry results
