"""Who owns a matrix handle's device memory: every layout sh_csr_upload_ex can build is released by sh_csr_free, a layout
that autotune drops leaves the footprint as well as the device, and the footprint of every layout is what it was before
the handle's arrays got one owner per layout.

The small matrix is R-MAT scale 12 (4096 rows), as in test_bits_gpu.py's leak test; forced options reach every path at
that size.  Free device memory is the device's own reading (Engine.max_alloc), so 16 MiB are allowed for what else
happens on it, as there."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from sparseharness_amd.engine import Engine

pytestmark = pytest.mark.gpu

N = 1 << 12
ALLOWANCE = 16 << 20
# name -> (upload options, int32 values, one reporting sh_spmv_step_pieces launch as well)
VARIANTS = {
    "stream": (dict(plan=1), False, False),
    "tiled-host": (dict(plan=2, build=1), False, True),
    "tiled-device-placed": (dict(plan=2, build=2, placement_tries=3), False, True),   # adopted arrays, swapped by placement
    "tiled-bits-beside": (dict(plan=2, or_and_bits=1), True, True),
    "bits-only": (dict(or_and_bits=2), True, False),
    "bits-only-device": (dict(or_and_bits=2, build=2), True, False),
}
# footprint() and describe() of the variants as the parent commit of the one-owner-per-layout refactor reported them on
# an MI355X (recorded from a run of that commit's engine, not from the code under test)
TILED = "tiled values=dict4(16) tiles=1 chunks=24 bins=2 heavy_rows=13 stream=0.1M light=0.1M products=0.0M folded"
PARENT = {
    "stream": (540852, "stream values=raw blocks=17 long_rows=0 segments=0 device=0.001GB"),
    "tiled-host": (355358, TILED + " device=0.000GB"),
    "tiled-device-placed": (355358, TILED + " device=0.000GB"),
    "tiled-bits-beside": (716074, TILED + " or_and=bits(items=1,entries=0.1M) device=0.001GB"),
    "bits-only": (360716, "bits-only or_and=bits(items=1,entries=0.1M,only) device=0.000GB"),
    "bits-only-device": (360716, "bits-only or_and=bits(items=1,entries=0.1M,only) device=0.000GB"),
}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _no_plan_in_the_environment(monkeypatch):
    for name in ("SH_PLAN", "SH_AUTOTUNE", "SH_BUILD", "SH_OR_AND_BITS", "SH_PLACEMENT_TRIES"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def small():
    rp, ci, va = H.rmat(12, seed=3)
    x = (1 + np.arange(N) % 7).astype(np.float32)
    data = {"rp": rp, "ci": ci, "f": va.astype(np.float32), "i": va.astype(np.int32), "xf": x, "xi": (np.arange(N) % 3 == 0).astype(np.int32)}
    for a in data.values():
        a.setflags(write=False)
    return data


def report_once(eng, sr, A, xv, out):
    """One sh_spmv_step_pieces launch with report = 1 (one piece over all rows): the piece state of the handle exists."""
    lib = abi.load()
    pc = abi.sh_row_pieces()
    pc.n_pieces, pc.piece_rows, pc.report, pc.gate = 1, N, 1, None
    pc.element_of_piece[0] = 0
    dt = np.float32 if sr == O.PLUS_TIMES_F32 else np.int32
    a, b = np.array([1], dt), np.array([0], dt)
    rnd, words = C.c_uint32(0), C.POINTER(C.c_uint32)()
    rc = lib.sh_spmv_step_pieces(eng.h, sr, A.h, xv.h, None, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.h,
                                 C.byref(pc), 0.25, None, C.byref(rnd), C.byref(words))
    assert rc == 0 and rnd.value == 1, (rc, rnd.value, lib.sh_last_error(eng.h))
    eng.synchronize()
    assert words[0] == 1


def cycle(eng, small, name, xv, out):
    """Upload, one launch (and one reporting launch where the variant asks for it), free -> (footprint, describe)."""
    opts, ints, pieces = VARIANTS[name]
    sr = O.OR_AND_I32 if ints else O.PLUS_TIMES_F32
    A = eng.upload_csr(N, N, small["rp"], small["ci"], small["i" if ints else "f"], **opts)
    seen = A.footprint(), A.describe()
    if "placement_tries" in opts:
        assert A.placement()[0] == opts["placement_tries"]
    eng.spmv(sr, A, xv, None, 1, 0, out)
    if pieces:
        report_once(eng, sr, A, xv, out)
    A.free()
    return seen


@pytest.fixture(scope="module")
def seen(eng, small):
    """(footprint, describe) of every variant, from one cycle each: also the warm-up of the leak test (code objects
    loaded, rocPRIM's and the engine's own state allocated)."""
    got = {}
    for name, (_, ints, _) in VARIANTS.items():
        xv, out = eng.vector(small["xi" if ints else "xf"]), eng.alloc(N)
        got[name] = cycle(eng, small, name, xv, out)
        xv.free()
        out.free()
    return got


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_footprint_and_description_are_the_parent_commits(seen, name):
    print(name, seen[name])
    assert seen[name] == PARENT[name]


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_upload_launch_free_cycles_do_not_grow_device_memory(eng, small, seen, name):
    """As many cycles as make the smallest footprint among the variants add up to eight times the allowance: a cycle
    that loses an eighth of its matrix fails."""
    smallest = min(fp for fp, _ in seen.values())
    cycles = -(-8 * ALLOWANCE // smallest)
    xv, out = eng.vector(small["xi" if VARIANTS[name][1] else "xf"]), eng.alloc(N)
    eng.synchronize()
    before = eng.max_alloc()
    for _ in range(cycles):
        assert cycle(eng, small, name, xv, out) == seen[name]
    eng.synchronize()
    after = eng.max_alloc()
    xv.free()
    out.free()
    print(f"{name}: {cycles} cycles of {seen[name][0]} bytes, free device memory before {before >> 20} MiB, after {after >> 20} MiB")
    assert before - after < ALLOWANCE, (before, after)


def test_a_dropped_layout_leaves_the_footprint(eng):
    """The smallest banded matrix the auto rule times (nnz >= 2^22, cols > 2^20, tile fill < 0.5): whichever plan the
    timing keeps, the handle accounts for that plan's arrays alone, exactly as a forced upload of that plan does."""
    rng = np.random.default_rng(5)
    n, per_row = (1 << 20) + 1, 4
    rp = (np.arange(n + 1, dtype=np.int64) * per_row).astype(np.int32)
    ci = (np.repeat(np.arange(n, dtype=np.int64), per_row) + rng.integers(-300, 301, n * per_row)).clip(0, n - 1).astype(np.int32)
    va = rng.integers(1, 17, n * per_row).astype(np.float32)
    x = (1 + np.arange(n) % 7).astype(np.float32)
    auto = eng.upload_csr(n, n, rp, ci, va, plan=0)
    d = auto.describe()
    assert "tuned(stream=" in d, d
    forced = {"stream": eng.upload_csr(n, n, rp, ci, va, plan=1), "tiled": eng.upload_csr(n, n, rp, ci, va, plan=2, placement_tries=1)}
    kept = auto.plan()[0]
    print(d, {k: A.footprint() for k, A in forced.items()}, auto.footprint())
    assert forced[kept].plan()[0] == kept
    assert auto.footprint() == forced[kept].footprint(), (d, kept)
    xv, out = eng.vector(x), eng.alloc(n).fill(0)
    eng.spmv(O.PLUS_TIMES_F32, auto, xv, None, 1.0, 0.0, out)
    np.testing.assert_array_equal(out.download(np.float32).view(np.uint32), O.gold_dot(rp, ci, va, x).view(np.uint32))
    for v in (xv, out):
        v.free()
    for A in (auto, *forced.values()):
        A.free()
