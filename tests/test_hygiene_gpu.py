"""What a dense launch may read and write: its operands, and scratch that it wrote itself.  GPU AddressSanitizer's class of
error, caught by construction instead: every comparison is == on the 32-bit words against the oracle's result
(tests/hygiene_shapes.py; tests/test_hygiene_cpu.py proves that a poison word reaching a row changes that row).

Tier 1, the production library:
  1. history -- one matrix handle launched with x_A, x_B, x_0, x_A, x_B: every column tile goes live -> dead -> live, so
     a launch that reads what the launch before left (a product of a tile that is dead now, a stale partial, a stale
     live word) gives another answer than the oracle.
  2. guards and alignment -- every operand is a view (sh_vec_wrap) into a larger allocation, GUARD words of the
     semiring's poison (inputs) or 0xDEADBEEF (outputs) on either side, starting at every word offset modulo 4: the
     result is the oracle's and no guard word changed.  The entry points that want 16-byte aligned vectors run at
     offsets 0 and 4 and refuse offset 1 without writing anything.
Tier 2, the tools library (sh_debug_poison_scratch, sh_debug_poison_loop_words):
  3. the sequence of 1 with every per-launch scratch array of the matrix filled with the semiring's poison before
     every launch, the tiles' live words with 0 and with 1, the marked piece table with and without PIECE_DEAD.
  4. the iteration loops with the device halves of their flag words filled before the call.

sh_iterate needs a square matrix, which the tiled shapes are not: it runs on the stream shape (across its long row) and
on the path with chords, each under both plans, and under the tiled plan on a path of 2 * 32760 + 3 vertices (two full
column tiles and one of three columns) with sources on both sides of each tile seam."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import hygiene_shapes as S
from guarded import DEAD, Dev, _not_halted, same_bits, vp   # noqa: F401 (the fixture is used by being here)
from oracle import oracle as O
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine
from test_plan_limits_gpu import Tools

pytestmark = pytest.mark.gpu

VARIANTS = {"stream": dict(plan=1), "tiled": dict(plan=2), "tiled-8bit": dict(plan=2, value_coding=8),
            "tiled-raw": dict(plan=2, value_coding=-1), "tiled-nofold": dict(plan=2, fold=0)}
_t0 = time.time()


def scalar(sr, v):
    return np.array([v], O.elem_dtype(sr))


class Operands:
    """x, y and an output prefilled with 0xDEADBEEF, each guarded; inputs between the semiring's poison."""

    def __init__(self, dev, sr, x, y, n_out, kx=0, ky=0, kout=None):
        self.x = dev.guarded(x, kx, S.POISON[sr])
        self.y = dev.guarded(y, ky, S.POISON[sr])
        self.out = dev.guarded(np.full(n_out, DEAD, np.uint32), ky if kout is None else kout, DEAD)
        self.x0, self.y0 = S.bits(x).ravel().copy(), S.bits(y).ravel().copy()

    def inputs_unchanged(self, what, x_too=True):
        if x_too:
            same_bits(self.x.read(what + " x"), self.x0, what + ": x was written")
        same_bits(self.y.read(what + " y"), self.y0, what + ": y was written")

    def free(self):
        for g in (self.x, self.y, self.out):
            g.free()


# ------------------------------------------------------------------ the two engines
@pytest.fixture(scope="module")
def prod():
    eng = Engine(0)
    d = Dev(abi.load(), eng.h)
    yield d
    d.close()
    eng.close()
    print(f"tests/test_hygiene_gpu.py: {time.time() - _t0:.1f} s since import")


@pytest.fixture(scope="module")
def tools():
    t = Tools()
    lib = t.lib
    lib.sh_debug_poison_scratch.restype = C.c_int
    lib.sh_debug_poison_scratch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_int64)]
    lib.sh_debug_poison_loop_words.restype = C.c_int
    lib.sh_debug_poison_loop_words.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64)]
    d = Dev(lib, t.e)
    yield d
    d.close()
    t.close()


def shape_matrix(dev, sr, shape, vset, **options):
    """The matrix of a shape with the values of the semiring's element type (two semirings share each)."""
    kind = "int" if S.is_int(sr) else "float"
    return dev.matrix((shape, vset, kind), lambda: S.pattern(shape) + (S.values_for(sr, shape, vset),), **options)


def spmv(dev, sr, A, ops, what):
    a, b = (scalar(sr, v) for v in S.SCALARS[sr])
    dev.ok(dev.lib.sh_spmv(dev.h, sr, A, ops.x.v, ops.y.v, vp(a), vp(b), ops.out.v, None, None))
    return ops.out.read(what + " out")


def run_sequence(dev, sr, A, shape, vset, what, before=None, kx=0, ky=0):
    """x_A, x_B, x_0, x_A, x_B on one handle, fresh guarded operands per launch: every result is the oracle's."""
    rows = S.pattern(shape)[0]
    for k, which in enumerate(S.SEQUENCE):
        w = f"{what}, launch {k} (x_{which})"
        ops = Operands(dev, sr, S.x_vector(sr, shape, which), S.y_vector(sr, rows), rows, kx, ky)
        try:
            if before:
                before(sr, A, w)
            same_bits(spmv(dev, sr, A, ops, w), S.want(sr, shape, vset, which), w)
            ops.inputs_unchanged(w)
        finally:
            ops.free()


def assert_layout(dev, A, shape, variant):
    d = dev.describe(A)
    if variant.startswith("tiled"):
        assert d.startswith("tiled") and "heavy_rows=2" in d and f"tiles={2 if shape == 'tiled2' else 3} " in d, d
        assert int(re.search(r"bins=(\d+)", d).group(1)) >= 3, d
        assert ("folded" in d) == (variant != "tiled-nofold"), d
    else:
        assert d.startswith("stream"), d
        if shape == "stream":
            assert int(re.search(r"long_rows=(\d+)", d).group(1)) >= 1 and int(re.search(r"segments=(\d+)", d).group(1)) >= 3, d


# ------------------------------------------------------------------ 1. history
@pytest.mark.parametrize("variant,build", [(v, b) for v in sorted(VARIANTS) for b in ("host", "device")
                                           if (v, b) != ("stream", "device")])   # (the CSR-stream layout has one builder)
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_history_of_a_handle_does_not_reach_its_next_launch(prod, shape, variant, build):
    for sr in S.SEMIRINGS:
        A = shape_matrix(prod, sr, shape, "nibble16", build=2 if build == "device" else 1, **VARIANTS[variant])
        assert_layout(prod, A, shape, variant)
        if variant != "stream":
            assert prod.builder(A) == build
        run_sequence(prod, sr, A, shape, "nibble16", f"{S.SR_NAME[sr]} {shape} {variant} {build}-built")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_history_on_the_bit_blocked_layout(prod, shape, mode):
    A = shape_matrix(prod, S.OA, shape, "nibble16", plan=2, build=1, or_and_bits=mode)
    d = prod.describe(A)
    assert "or_and=bits(" in d and ("only" in d) == (mode == 2), d
    run_sequence(prod, S.OA, A, shape, "nibble16", f"or_and {shape} or_and_bits={mode}")


def offsets_of(offset, misplace):
    """(kx, ky, kout): all at `offset`, the operand named by `misplace` one word off a 16-byte boundary."""
    return tuple(1 if misplace == name else offset for name in ("x", "y", "out"))


def spmm(dev, sr, A, width, k, what, offset=0, before=None, expect=abi.SH_OK, misplace=None):
    X, Y, W = S.spmm_case(sr, width, k)
    ops = Operands(dev, sr, X, Y, W.size, *offsets_of(offset, misplace))
    try:
        if before:
            before(sr, A, what)
        a, b = (scalar(sr, v) for v in S.SCALARS[sr])
        rc = dev.lib.sh_spmm(dev.h, sr, A, width, ops.x.v, ops.y.v, vp(a), vp(b), ops.out.v, None)
        if expect != abi.SH_OK:
            assert rc == expect, (what, rc)
            assert (ops.out.read(what + " out") == DEAD).all(), what + ": a refused call wrote to Out"
        else:
            dev.ok(rc)
            same_bits(ops.out.read(what + " out"), W, what)
        ops.inputs_unchanged(what)
    finally:
        ops.free()


def bits_spmv(dev, A, words, k, what, offset=0, before=None, expect=abi.SH_OK, misplace=None):
    X, Y, W = S.bits_case(words, k)
    ops = Operands(dev, S.OA, X, Y, W.size, *offsets_of(offset, misplace))
    try:
        if before:
            before(S.OA, A, what)
        a, b = scalar(S.OA, 1), scalar(S.OA, 1)
        rc = dev.lib.sh_bits_spmv(dev.h, A, words, ops.x.v, ops.y.v, vp(a), vp(b), ops.out.v, None)
        if expect != abi.SH_OK:
            assert rc == expect, (what, rc)
            assert (ops.out.read(what + " out") == DEAD).all(), what + ": a refused call wrote to Out"
        else:
            dev.ok(rc)
            same_bits(ops.out.read(what + " out"), W, what)
        ops.inputs_unchanged(what)
    finally:
        ops.free()


def stream_matrix(dev, sr):
    A = shape_matrix(dev, sr, "stream", "nibble16", plan=1)
    assert_layout(dev, A, "stream", "stream")
    return A


@pytest.mark.parametrize("width", [4, 32])
@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_history_of_spmm_across_the_long_row(prod, sr, width):
    A = stream_matrix(prod, sr)
    for k in range(len(S.SEQUENCE)):
        spmm(prod, sr, A, width, k, f"sh_spmm {S.SR_NAME[sr]} width {width}, launch {k}")


@pytest.mark.parametrize("words", [1, 8])
def test_history_of_bits_spmv_across_the_long_row(prod, words):
    A = stream_matrix(prod, S.OA)
    for k in range(len(S.SEQUENCE)):
        bits_spmv(prod, A, words, k, f"sh_bits_spmv words {words}, launch {k}")


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_history_of_spmv_across_the_long_row(prod, sr):
    run_sequence(prod, sr, stream_matrix(prod, sr), "stream", "nibble16", f"{S.SR_NAME[sr]} stream shape")


# ------------------------------------------------------------------ 2. guards and alignment
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("shape", S.SHAPES)
def test_spmv_on_views_at_every_word_offset(prod, shape, k):
    """x starts k words behind a 16-byte boundary, y and out (k + 1) % 4: at k = 0 the full tiles of x are staged by
    16-byte loads, at every other k word by word, and the last tile of "tiled3" word by word in any case."""
    variant = "stream" if shape == "stream" else "tiled"
    for sr in S.SEMIRINGS:
        A = shape_matrix(prod, sr, shape, "nibble16", build=1, **VARIANTS[variant])
        assert_layout(prod, A, shape, variant)
        run_sequence(prod, sr, A, shape, "nibble16", f"{S.SR_NAME[sr]} {shape} x at word {k}", kx=k, ky=(k + 1) % 4)
    if shape in S.TILED:   # bits_pack_x reads x four words at a time when it is 16-byte aligned, word by word otherwise
        for mode in (1, 2):
            A = shape_matrix(prod, S.OA, shape, "nibble16", plan=2, build=1, or_and_bits=mode)
            assert "or_and=bits(" in prod.describe(A)
            run_sequence(prod, S.OA, A, shape, "nibble16", f"or_and {shape} or_and_bits={mode} x at word {k}", kx=k, ky=(k + 1) % 4)


def loop_matrix(dev, sr, plan):
    def make():
        n, rp, ci = S.loop_graph()
        return n, n, rp, ci, S.loop_values(sr)
    A = dev.matrix(("loop", S.SR_NAME[sr]), make, plan=plan)
    assert dev.describe(A).startswith("stream" if plan == 1 else "tiled"), dev.describe(A)
    return A


def iterate(dev, sr, A, x0, cap, what, kx=0, ky=0, before=None):
    """sh_iterate on guarded x, y0 and scratch -> (vector, launches, converged)."""
    n = len(x0)
    ops = Operands(dev, sr, x0, x0, n, kx, ky)
    try:
        if before:
            before(what)
        a, b = (scalar(sr, v) for v in S.LOOP_SCALARS[sr])
        iters, conv = C.c_int32(-1), C.c_int32(-1)
        dev.ok(dev.lib.sh_iterate(dev.h, sr, A, ops.x.v, ops.y.v, ops.out.v, vp(a), vp(b), S.DELTA, cap, None, C.byref(iters),
                                  C.byref(conv), None, None))
        got = ops.x.read(what + " x")
        ops.out.read(what + " scratch")
        ops.inputs_unchanged(what, x_too=False)
        return got, iters.value, bool(conv.value)
    finally:
        ops.free()


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("sr", (S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_iterate_on_views_at_every_word_offset(prod, sr, k):
    """x at word k, y0 and scratch at (k + 1) % 4 (the loop reads x and scratch in turn, so both offsets are staged)."""
    ky = (k + 1) % 4
    # the stream shape: the long row's segments and its fix-up run, gated, in every launch of the loop
    rows, cols, rp, ci = S.pattern("stream")
    va, x0, want, w_it, w_conv = S.stream_loop(sr)
    for plan in (1, 2):
        A = prod.matrix(("stream_loop", S.SR_NAME[sr]), lambda: (rows, cols, rp, ci, va), plan=plan, build=1)
        d = prod.describe(A)
        if plan == 1:
            assert_layout(prod, A, "stream", "stream")
        else:
            assert d.startswith("tiled") and int(re.search(r"heavy_rows=(\d+)", d).group(1)) >= 1, d
        what = f"sh_iterate {S.SR_NAME[sr]} plan={plan} stream shape, x at word {k}"
        got, it, conv = iterate(prod, sr, A, x0, S.STREAM_CAP, what, k, ky)
        assert (it, conv) == (w_it, w_conv), (what, it, conv)
        same_bits(got, want, what)
    # the path with chords: 89 launches
    for plan in (1, 2):
        A = loop_matrix(prod, sr, plan)
        want, w_it, w_conv = S.loop_ref(sr, 0)
        what = f"sh_iterate {S.SR_NAME[sr]} plan={plan} path with chords, x at word {k}"
        got, it, conv = iterate(prod, sr, A, S.loop_start(sr, 0), S.LOOP_CAP, what, k, ky)
        assert (it, conv) == (w_it, w_conv) and it > 16, (what, it, conv)
        same_bits(got, want, what)
    # 20 launches (three batches) over three column tiles, every tile live in every launch (tests/test_hygiene_cpu.py):
    # stopped by the cap, as the oracle is
    n, rp, ci = S.long_path()
    va, x0 = S.long_case(sr)
    A = prod.matrix(("long_path", S.SR_NAME[sr]), lambda: (n, n, rp, ci, va), plan=2, build=1)
    assert prod.describe(A).startswith("tiled") and "tiles=3 " in prod.describe(A)
    want, w_it, w_conv = S.long_ref(sr)
    what = f"sh_iterate {S.SR_NAME[sr]} tiled path of {n}, x at word {k}"
    got, it, conv = iterate(prod, sr, A, x0, S.LONG_CAP, what, k, ky)
    assert (it, conv) == (w_it, w_conv) == (S.LONG_CAP, False), (what, it, conv)
    same_bits(got, want, what)


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_spmm_on_views_aligned_and_refused(prod, sr):
    A = stream_matrix(prod, sr)
    for width in (4, 32):
        for offset in (0, 4):
            spmm(prod, sr, A, width, 0, f"sh_spmm {S.SR_NAME[sr]} width {width} at word {offset}", offset)
    for which in ("x", "y", "out"):
        spmm(prod, sr, A, 4, 0, f"sh_spmm {S.SR_NAME[sr]} with {which} at word 1", 0, expect=abi.SH_EINVAL, misplace=which)


def test_bits_spmv_on_views_aligned_and_refused(prod):
    A = stream_matrix(prod, S.OA)
    for words in (1, 8):
        for offset in (0, 4):
            bits_spmv(prod, A, words, 0, f"sh_bits_spmv words {words} at word {offset}", offset)
    for which in ("x", "y", "out"):
        bits_spmv(prod, A, 1, 0, f"sh_bits_spmv with {which} at word 1", 0, expect=abi.SH_EINVAL, misplace=which)


def iterate_multi(dev, sr, A, width, what, offset=0, before=None, expect=abi.SH_OK):
    n = S.LOOP_N
    X0 = np.ascontiguousarray(np.stack([S.loop_start(sr, v) for v in S.LOOP_SOURCES[:width]], axis=1))
    ops = Operands(dev, sr, X0, X0, X0.size, offset, 0 if expect != abi.SH_OK else offset)
    try:
        if before:
            before(what)
        a, b = (scalar(sr, v) for v in S.LOOP_SCALARS[sr])
        launches = C.c_int32(-1)
        iters, conv = (C.c_int32 * width)(), (C.c_int32 * width)()
        rc = dev.lib.sh_iterate_multi(dev.h, sr, A, width, ops.x.v, ops.y.v, ops.out.v, vp(a), vp(b), S.DELTA, S.LOOP_CAP,
                                      C.byref(launches), iters, conv, None, None)
        if expect != abi.SH_OK:
            assert rc == expect, (what, rc)
            same_bits(ops.x.read(what + " X"), X0, what + ": a refused call wrote to X")
            assert (ops.out.read(what + " scratch") == DEAD).all(), what + ": a refused call wrote to scratch"
            return
        dev.ok(rc)
        got = ops.x.read(what + " X").reshape(n, width)
        ops.out.read(what + " scratch")
        ops.inputs_unchanged(what, x_too=False)
        refs = [S.loop_ref(sr, v) for v in S.LOOP_SOURCES[:width]]
        assert list(iters) == [r[1] for r in refs] and list(conv) == [int(r[2]) for r in refs], (what, list(iters), list(conv))
        assert launches.value == max(iters) > 16, (what, launches.value)
        for j in range(width):
            same_bits(got[:, j], refs[j][0], f"{what} column {j}")
    finally:
        ops.free()


def bits_iterate(dev, A, words, what, offset=0, before=None, expect=abi.SH_OK):
    n, n_src = S.LOOP_N, 32 * words
    src = [S.LOOP_SOURCES[s % len(S.LOOP_SOURCES)] for s in range(n_src)]
    P0 = S.pack(np.stack([S.loop_start(S.OA, v) for v in src], axis=1), words)
    refs = [S.loop_ref(S.OA, v) for v in src]
    cap = max(r[1] for r in refs) + 3
    ops = Operands(dev, S.OA, P0, P0, P0.size, offset, 0 if expect != abi.SH_OK else offset)
    try:
        if before:
            before(what)
        a, b = scalar(S.OA, 1), scalar(S.OA, 1)
        launches = C.c_int32(-1)
        iters, conv = (C.c_int32 * n_src)(), (C.c_int32 * n_src)()
        newly = np.full((cap, n_src), 0x5A5A5A5A, np.uint32)
        rc = dev.lib.sh_bits_iterate(dev.h, A, words, ops.x.v, ops.y.v, ops.out.v, vp(a), vp(b), cap, C.byref(launches), iters, conv,
                                     newly.ctypes.data_as(C.POINTER(C.c_uint32)), None, None)
        if expect != abi.SH_OK:
            assert rc == expect, (what, rc)
            same_bits(ops.x.read(what + " X"), P0, what + ": a refused call wrote to X")
            assert (ops.out.read(what + " scratch") == DEAD).all(), what + ": a refused call wrote to scratch"
            return
        dev.ok(rc)
        got = ops.x.read(what + " X").reshape(n, words)
        ops.out.read(what + " scratch")
        ops.inputs_unchanged(what, x_too=False)
        assert list(iters) == [r[1] for r in refs] and list(conv) == [int(r[2]) for r in refs], (what, list(iters)[:8], list(conv)[:8])
        assert launches.value == max(iters) > 16, (what, launches.value)
        same_bits(got, S.pack(np.stack([r[0] for r in refs], axis=1), words), what)
        levels = np.zeros((cap, n_src), np.uint32)
        for s, v in enumerate(src):
            sizes = S.loop_levels(v)
            levels[:len(sizes), s] = sizes
        assert np.array_equal(newly, levels), (what, np.argwhere(newly != levels)[:6].tolist())
    finally:
        ops.free()


@pytest.mark.parametrize("sr", (S.MP, S.OA), ids=S.SR_NAME.get)
def test_iterate_multi_on_views_aligned_and_refused(prod, sr):
    A = loop_matrix(prod, sr, 1)
    for offset in (0, 4):
        iterate_multi(prod, sr, A, 8, f"sh_iterate_multi {S.SR_NAME[sr]} width 8 at word {offset}", offset)
    iterate_multi(prod, sr, A, 8, f"sh_iterate_multi {S.SR_NAME[sr]} with X at word 1", 1, expect=abi.SH_EINVAL)


def test_bits_iterate_on_views_aligned_and_refused(prod):
    A = loop_matrix(prod, S.OA, 1)
    for offset in (0, 4):
        bits_iterate(prod, A, 1, f"sh_bits_iterate words 1 at word {offset}", offset)
    bits_iterate(prod, A, 1, "sh_bits_iterate with X at word 1", 1, expect=abi.SH_EINVAL)


# ------------------------------------------------------------------ 3. poisoned scratch
_printed = set()
NAMES = ("P", "tpartial", "tile_live", "ptab_live", "partial", "partial_multi", "xbits", "bits_partial")


def poisoner(dev, live_word, dead_piece, owns, exact=None):
    """-> before(sr, A, what): fills the matrix's scratch with the semiring's poison and asserts that exactly the arrays
    of `owns` exist (a pass over an array of 0 bytes is no pass); exact: {name: bytes}."""
    def before(sr, A, what):
        sizes = (C.c_int64 * 8)(*([-1] * 8))
        dev.ok(dev.lib.sh_debug_poison_scratch(dev.h, A, S.POISON[sr], live_word, dead_piece, sizes))
        got = dict(zip(NAMES, sizes))
        if (A.value, dead_piece) not in _printed:
            _printed.add((A.value, dead_piece))
            print(f"{what}: bytes poisoned {got}")
        want_owned = set(owns) - ({"ptab_live"} if not dead_piece else set())
        assert {n for n, b in got.items() if b > 0} == want_owned and min(got.values()) >= 0, (what, got)
        for name, b in (exact or {}).items():
            assert got[name] == b, (what, name, got[name], b)
    return before


TILED_OWNS = ("P", "tpartial", "tile_live", "ptab_live")
PASSES = [(live, dead) for live in (0, 1) for dead in (0, 1)]


def tiled_exact(dev, A, shape):
    tiles = 2 if shape == "tiled2" else 3
    return {"P": max(dev.lib.sh_debug_p_len(A), 4) * 4 + 16, "tile_live": tiles * 4}


@pytest.mark.parametrize("fold,vset", [(1, v) for v in sorted(S.VALUE_SETS)] + [(0, "nibble16")])
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_poisoned_scratch_of_the_tiled_plan(tools, shape, vset, fold):
    for sr in S.SEMIRINGS:
        A = shape_matrix(tools, sr, shape, vset, plan=2, build=1, fold=fold)
        assert_layout(tools, A, shape, "tiled" if fold else "tiled-nofold")
        coding = {4: "dict4", 8: "dict8", 16: "dict16", 0: "raw"}[S.VALUE_SETS[vset][1]]
        assert f"values={coding}" in tools.describe(A), tools.describe(A)
        for live_word, dead_piece in PASSES:
            before = poisoner(tools, live_word, dead_piece, TILED_OWNS, tiled_exact(tools, A, shape))
            run_sequence(tools, sr, A, shape, vset, f"{S.SR_NAME[sr]} {shape} {vset} fold={fold} live_word={live_word} dead_piece={dead_piece}", before)


@pytest.mark.parametrize("sr", S.SEMIRINGS, ids=S.SR_NAME.get)
def test_poisoned_scratch_of_the_stream_plan(tools, sr):
    A = stream_matrix(tools, sr)
    before = poisoner(tools, 0, 0, ("partial", "partial_multi"))
    run_sequence(tools, sr, A, "stream", "nibble16", f"{S.SR_NAME[sr]} stream shape, poisoned", before)
    for width in (4, 32):
        for k in range(len(S.SEQUENCE)):
            spmm(tools, sr, A, width, k, f"sh_spmm {S.SR_NAME[sr]} width {width}, launch {k}, poisoned", before=before)
    if sr == S.OA:
        for words in (1, 8):
            for k in range(len(S.SEQUENCE)):
                bits_spmv(tools, A, words, k, f"sh_bits_spmv words {words}, launch {k}, poisoned", before=before)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", sorted(S.TILED))
def test_poisoned_scratch_of_the_bit_blocked_layout(tools, shape, mode):
    A = shape_matrix(tools, S.OA, shape, "nibble16", plan=2, build=1, or_and_bits=mode)
    owns = ("xbits", "bits_partial") + (TILED_OWNS if mode == 1 else ())
    for live_word, dead_piece in PASSES:
        before = poisoner(tools, live_word, dead_piece, owns)
        run_sequence(tools, S.OA, A, shape, "nibble16", f"or_and {shape} or_and_bits={mode} live_word={live_word} dead_piece={dead_piece}", before)


# ------------------------------------------------------------------ 4. poisoned loop words
LOOP_WORDS = (0xFFFFFFFF, 0x00000000, 0x00000001)


LOOP_BYTES = {"flags": 64, "mflags": (8 + 1) * 32 * 4, "bstate": ((8 + 1) * 8 + 8 * 256) * 4}   # as the loops open them


def loop_poisoner(dev, word, uses):
    """-> before(what): fills the loop words that are open; the array the loop under test uses must have been filled
    with all its bytes (a pass over an array of 0 bytes is no pass)."""
    def before(what):
        sizes = (C.c_int64 * 3)(-1, -1, -1)
        dev.ok(dev.lib.sh_debug_poison_loop_words(dev.h, word, sizes))
        got = dict(zip(("flags", "mflags", "bstate"), sizes))
        assert got[uses] == LOOP_BYTES[uses] and all(b in (0, LOOP_BYTES[n]) for n, b in got.items()), (what, got)
    return before


@pytest.mark.parametrize("sr", (S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_iterate_with_poisoned_flag_words(tools, sr):
    for plan in (1, 2):
        A = loop_matrix(tools, sr, plan)
        want, w_it, w_conv = S.loop_ref(sr, 0)
        for word in (None,) + LOOP_WORDS:   # (the first run opens the words)
            what = f"sh_iterate {S.SR_NAME[sr]} plan={plan}, loop words {word}"
            got, it, conv = iterate(tools, sr, A, S.loop_start(sr, 0), S.LOOP_CAP, what, before=None if word is None else loop_poisoner(tools, word, "flags"))
            assert (it, conv) == (w_it, w_conv) and it > 16, (what, it, conv)
            same_bits(got, want, what)


@pytest.mark.parametrize("sr", (S.MP, S.OA), ids=S.SR_NAME.get)
def test_iterate_multi_with_poisoned_flag_words(tools, sr):
    A = loop_matrix(tools, sr, 1)
    for word in (None,) + LOOP_WORDS:
        iterate_multi(tools, sr, A, 8, f"sh_iterate_multi {S.SR_NAME[sr]} width 8, loop words {word}",
                      before=None if word is None else loop_poisoner(tools, word, "mflags"))


@pytest.mark.parametrize("words", [1, 8])
def test_bits_iterate_with_poisoned_state_words(tools, words):
    A = loop_matrix(tools, S.OA, 1)
    for word in (None,) + LOOP_WORDS:
        bits_iterate(tools, A, words, f"sh_bits_iterate words {words}, loop words {word}",
                     before=None if word is None else loop_poisoner(tools, word, "bstate"))
