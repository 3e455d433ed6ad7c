"""The phase-1 work items of the x-tiled plan (plan_common.h::cut_work_items), without a GPU: the host builder's
item list for 8, 32 and 256 CUs with the end of every XCD's list re-cut (the default) and plain (SH_P1_TAIL=0), and
the host emulator's result through either list.  The tools build exports sh_debug_plan_items for it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import p1_items_shapes as S
from sparseharness_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparseharness_amd", "csrc")
LIB = os.path.join(ROOT, "sparseharness_amd", "variants", "emulate.so")
CAP = 1 << 14


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", CSRC, "emulate"])   # (rebuilds only when a source is newer)
    lib = C.CDLL(LIB)
    lib.sh_plan_options_default.argtypes = [C.POINTER(abi.sh_plan_options)]
    lib.sh_debug_plan_items.restype = C.c_int64
    lib.sh_debug_plan_items.argtypes = ([C.c_int64] * 3 + [C.c_void_p] * 3 + [C.POINTER(abi.sh_plan_options), C.c_int, C.c_int]
                                        + [C.c_void_p] * 4 + [C.c_int64])
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def cases():
    """name -> the matrix, x and the exact product (float64 sums of exactly representable terms), computed once."""
    out = {}
    for name in S.SHAPES:
        rows, cols, rp, ci, va = S.matrix(name)
        x = S.x_float(cols)
        want = np.zeros(rows)
        np.add.at(want, np.repeat(np.arange(rows), np.diff(rp)), x[ci].astype(np.float64) * va.astype(np.float64))
        assert want.max() < 2 ** 24
        out[name] = (rows, cols, rp, ci, va, x, want.astype(np.float32))
    return out


def plan_items(lib, case, n_cus, tail, monkeypatch, **options):
    rows, cols, rp, ci, va, x, _ = case
    if tail:
        monkeypatch.delenv("SH_P1_TAIL", raising=False)
    else:
        monkeypatch.setenv("SH_P1_TAIL", "0")
    opt = abi.sh_plan_options()
    lib.sh_plan_options_default(C.byref(opt))
    opt.plan = 2
    for k, v in options.items():
        setattr(opt, k, v)
    items = np.zeros((CAP, 8), np.int32)
    y = np.zeros(rows, np.float32)
    st = np.zeros(8, np.int64)
    n = lib.sh_debug_plan_items(rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), n_cus, 0, _p(x), _p(y), _p(st), _p(items), CAP)
    assert 0 < n <= CAP, n
    return items[:n].copy(), y, st


def split(items):
    """(light items, heavy items) without the fillers; columns: tile, s, e, hs, pdelta, ob0."""
    real = items[items[:, 1] < items[:, 2]]
    heavy = real[:, 3] <= real[:, 1]
    return real[~heavy], real[heavy]


def covered(items):
    """The stream entries of the items as merged [s, e) intervals; asserts that no entry lies in two items."""
    real = items[items[:, 1] < items[:, 2]]
    real = real[np.argsort(real[:, 1], kind="stable")]
    assert (real[1:, 1] >= real[:-1, 2]).all(), "two items share stream entries"
    merged = []
    for s, e in real[:, 1:3].tolist():
        if merged and merged[-1][1] == s:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    return merged


@pytest.mark.parametrize("n_cus", [8, 32, 256])
@pytest.mark.parametrize("name", sorted(S.SHAPES))
def test_items_with_and_without_the_tail_policy(emu, cases, monkeypatch, name, n_cus):
    case = cases[name]
    plain, y_plain, st_plain = plan_items(emu, case, n_cus, False, monkeypatch)
    tail, y_tail, st_tail = plan_items(emu, case, n_cus, True, monkeypatch)
    # every stream entry in exactly one item: no overlap, the same entries as the plain list, and the emulator (which
    # fills P and the partial slots with poison first) read nothing that no item had written
    assert covered(tail) == covered(plain)
    assert st_plain[6] == 0 and st_tail[6] == 0
    for items in (plain, tail):
        light, heavy = split(items)
        # heavy cuts are whole waves of strips from the run's start (hs of a heavy item)
        assert ((heavy[:, 1] - heavy[:, 3]) % S.WAVE == 0).all()
        ends = {int(t): int(heavy[heavy[:, 0] == t][:, 2].max()) for t in set(heavy[:, 0].tolist())}
        for t, s, e in heavy[:, :3].tolist():
            assert (e - s) % S.WAVE == 0 or e == ends[t], "only the last item of a heavy run may end inside a wave"
        # position p holds an item of XCD p % 8: a tile's items all sit on one XCD's positions (uniform columns: tile % 8)
        pos = np.nonzero(items[:, 1] < items[:, 2])[0]
        assert (pos % 8 == items[pos, 0] % 8).all()
        assert len(items) % 8 == 0
    # the light items are the same ones (ob0 included), in the same order on every XCD's list
    for x in range(8):
        np.testing.assert_array_equal(split(tail[x::8])[0], split(plain[x::8])[0])
    # the emulator's result: the same bits either way, and the exact product
    np.testing.assert_array_equal(y_tail.view(np.uint32), y_plain.view(np.uint32))
    np.testing.assert_array_equal(y_tail, case[6])
    if n_cus == 8:   # one CU per XCD: nothing to balance
        np.testing.assert_array_equal(tail, plain)


@pytest.mark.parametrize("name,n_cus", [("one_tile", 32), ("nine_tiles_three_heavy", 256), ("eighth_shard", 32)])
def test_the_policy_moves_heavy_items_to_the_end_of_a_list(emu, cases, monkeypatch, name, n_cus):
    """Where it applies (heavy runs of several items, more than one CU per XCD) the list ends with heavy items, finer
    than the plain ones and longest first; a forced item size (chunk > 0) keeps the plain list."""
    case = cases[name]
    plain, _, _ = plan_items(emu, case, n_cus, False, monkeypatch)
    tail, _, _ = plan_items(emu, case, n_cus, True, monkeypatch)
    assert len(split(tail)[1]) > len(split(plain)[1])
    changed = n_recut = 0
    for x in range(8):
        lp, lt = plain[x::8], tail[x::8]
        lp, lt = lp[lp[:, 1] < lp[:, 2]], lt[lt[:, 1] < lt[:, 2]]
        if len(lp) == len(lt) and (lp == lt).all():
            continue
        changed += 1
        before = set(map(tuple, lp[:, 1:3].tolist()))
        recut = [k for k in range(len(lt)) if tuple(lt[k, 1:3].tolist()) not in before]   # the items the policy made
        if not recut:   # whole heavy items moved to the end, none of them cut
            continue
        n_recut += len(recut)
        assert (lt[recut, 3] <= lt[recut, 1]).all(), "only heavy items are cut again"
        assert (lt[recut, 2] - lt[recut, 1]).max() <= 49152 // 2
        last_light = max(k for k in range(len(lt)) if lt[k, 3] > lt[k, 1])
        assert recut[0] > last_light, "they stand behind every light item"
        size = lt[recut[0]:, 2] - lt[recut[0]:, 1]
        assert (size[1:] <= size[:-1]).all(), "longest first to the end of the list"
    assert changed > 0 and n_recut >= 2
    forced_plain, _, _ = plan_items(emu, case, n_cus, False, monkeypatch, chunk=49152)
    forced_tail, _, _ = plan_items(emu, case, n_cus, True, monkeypatch, chunk=49152)
    np.testing.assert_array_equal(forced_tail, forced_plain)
