"""The step BEFORE a tiled layout exists, without a GPU: where the host builder (plan_host.h::build_tiled_plan) refuses
a matrix, through the tools build's emulator (rc -1 = refused; an accepted matrix is walked through both phases and
compared with the CSR product).  The shapes are tests/plan_limit_shapes.py; the limit on the products in P
(plan_common.h::max_p_len: P is addressed with 32-bit byte offsets) is lowered through sh_debug_set_p_limit so that a
matrix of 36 K entries reaches it.  tests/test_plan_limits_gpu.py holds the device builder to the same verdicts."""
import ctypes as C

import numpy as np
import pytest

import plan_limit_shapes as S
from sparseharness_amd import abi
from test_plan_cpu import _p, emu, emulate, exact, random_matrix   # noqa: F401  (emu: the fixture that builds and loads emulate.so)


@pytest.fixture()
def lim(emu):
    emu.sh_debug_set_p_limit.restype = C.c_int64
    emu.sh_debug_set_p_limit.argtypes = [C.c_int64]
    yield emu
    emu.sh_debug_set_p_limit(0)


def verdict(lib, rows, cols, rp, ci, va, **options):
    """rc of the emulator alone.  (A refusal comes before the first use of x: the 2^31 - 1 column shape passes none.)"""
    opt = abi.sh_plan_options()
    lib.sh_plan_options_default(C.byref(opt))
    opt.plan = 2
    for k, v in options.items():
        setattr(opt, k, v)
    x = np.ones(cols, np.float32) if cols < 10 ** 8 else None
    y = np.zeros(rows, np.float32)
    return lib.sh_debug_emulate_plan(rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), 0, None if x is None else _p(x), _p(y), None)


@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_host_builder_refuses_exactly_the_shapes_beyond_a_limit(emu, name):
    make, built, _ = S.TABLE[name]
    rows, cols, rp, ci, va = make()
    if not built:
        assert verdict(emu, rows, cols, rp, ci, va) == -1
        return
    rc, y, st, x = emulate(emu, rows, cols, rp, ci, va, 0)
    assert rc == 0 and st["poison_reads"] == 0, (rc, st)
    np.testing.assert_array_equal(y, exact(rows, cols, rp, ci, va, x, 0))


def test_the_shapes_sit_where_the_rule_says():
    """The arithmetic of the 25 % rule on the shapes above, by hand: stream <= nnz + nnz / 4 + 4096 + 256 * tiles."""
    for bins, built in ((150, False), (60, True), (64, True), (65, False)):
        assert (S.light_stream_len(bins) <= S.stream_limit(62 * bins, 62)) == built, bins
    for nrows, built in ((100, False), (56, True), (57, False)):
        assert (S.heavy_stream_len(nrows) <= S.stream_limit(512 * nrows, 62)) == built, nrows
    assert (S.light_stream_len(64), S.stream_limit(62 * 64, 62)) == (15872, 24928)
    assert (S.heavy_stream_len(56), S.stream_limit(512 * 56, 62)) == (55552, 55808)
    assert (S.heavy_stream_len(57), S.stream_limit(512 * 57, 62)) == (56544, 56448)


def test_accepted_shapes_have_the_stream_length_the_arithmetic_gives(emu):
    for make, want in ((lambda: S.light_pieces(64), S.light_stream_len(64)), (lambda: S.heavy_strips(56), S.heavy_stream_len(56))):
        rows, cols, rp, ci, va = make()
        rc, _, st, _ = emulate(emu, rows, cols, rp, ci, va, 0)
        assert rc == 0 and st["stream"] == want, (rc, st, want)


@pytest.mark.parametrize("fold", [1, 0])
def test_p_limit_refuses_one_group_below_the_matrix_and_builds_at_it(lim, fold):
    rng = np.random.default_rng(101)
    rows, cols = 3000, 100_000
    rp, ci, va = random_matrix(rng, rows, cols, 12, 3)
    rc, y0, st, x = emulate(lim, rows, cols, rp, ci, va, 0, fold=fold)
    assert rc == 0
    p_len = st["products"]
    assert p_len > 0 and p_len % 4 == 0
    want = exact(rows, cols, rp, ci, va, x, 0)
    np.testing.assert_array_equal(y0, want)
    lim.sh_debug_set_p_limit(p_len)
    rc, y1, st1, _ = emulate(lim, rows, cols, rp, ci, va, 0, fold=fold)
    assert rc == 0 and st1 == st
    np.testing.assert_array_equal(y1, want)
    lim.sh_debug_set_p_limit(p_len - 4)
    assert verdict(lim, rows, cols, rp, ci, va, fold=fold) == -1
    lim.sh_debug_set_p_limit(-1)                                   # a negative value changes nothing
    assert verdict(lim, rows, cols, rp, ci, va, fold=fold) == -1
    lim.sh_debug_set_p_limit(0)                                    # the real bound again
    rc, y2, st2, _ = emulate(lim, rows, cols, rp, ci, va, 0, fold=fold)
    assert rc == 0 and st2 == st
    np.testing.assert_array_equal(y2, want)


def test_folding_changes_the_products_of_the_fixture(lim):
    """(what makes the two cases above two cases)"""
    rng = np.random.default_rng(101)
    rp, ci, va = random_matrix(rng, 3000, 100_000, 12, 3)
    p = [emulate(lim, 3000, 100_000, rp, ci, va, 0, fold=f)[2]["products"] for f in (1, 0)]
    assert p[0] < p[1], p


def test_the_real_bound_is_the_last_p_len_whose_dead_group_ends_below_4_gib(lim):
    """P holds max(p_len, 4) * 4 + 16 bytes (engine.hip) and phase 2 addresses all of them -- the dead-piece group behind
    the last product included -- with a 32-bit byte offset: the bound is the largest p_len (a multiple of 4) that fits."""
    bound = lim.sh_debug_set_p_limit(-1)
    assert bound % 4 == 0
    assert 4 * max(bound, 4) + 16 <= 2 ** 32
    assert 4 * max(bound + 4, 4) + 16 > 2 ** 32
    lim.sh_debug_set_p_limit(12345)
    assert lim.sh_debug_set_p_limit(-1) == bound                   # what it returns is the constant, not the override
