"""Where sh_csr_upload_ex decides whether a tiled layout may exist, and what happens when it may not -- on the GPU, through
the tools build of the engine (its own sh_engine, so that the sh_debug_* switches and the upload live in one library):
  (a) the host builder and the device builder give the same verdict on every shape of tests/plan_limit_shapes.py and on
      the limit of P (plan_common.h::max_p_len), and the device builder names the rule;
  (b) a forced plan = 2 that a limit rules out ends in a working CSR-stream matrix that keeps nothing of the abandoned build;
  (c) so does a matrix with more than 65535 column tiles (upload only: its x would be 8 GB);
  (d) a device build step that fails (sh_debug_fail_device_build) falls back to the host builder, same layout, same bits,
      nothing leaked.
Everything is exact: verdicts, strings, footprints, bits (small integer values, so (+,x) sums are exact in any order)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plan_limit_shapes as S
from oracle import oracle as O
from sparseharness_amd import abi
from sparseharness_amd import hostlib as H
from test_builder_gpu import random_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparseharness_amd", "csrc")
LIB = os.path.join(ROOT, "sparseharness_amd", "variants", "emulate.so")
SEMIRINGS = (O.PLUS_TIMES_F32, O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32)
SCALARS = {O.PLUS_TIMES_F32: (1.0, 0.5), O.MIN_PLUS_F32: (0.0, 0.0), O.OR_AND_I32: (1, 1), O.MAX_MIN_I32: (1, 1)}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Tools:
    """The tools library through ctypes: the product ABI (abi.SIGNATURES) plus the sh_debug_* hooks, and one engine."""

    def __init__(self):
        rc = subprocess.call(["make", "-s", "-C", CSRC, "emulate"])   # (rebuilds only when a source is newer than the library)
        assert rc == 0 or os.path.exists(LIB)
        try:
            import torch  # noqa: F401  (as abi.load(): torch's HIP runtime first, the engine then shares it)
        except ImportError:
            pass
        lib = self.lib = C.CDLL(LIB)
        for name, (res, args) in abi.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib.sh_debug_set_p_limit.restype, lib.sh_debug_set_p_limit.argtypes = C.c_int64, [C.c_int64]
        lib.sh_debug_fail_device_build.restype, lib.sh_debug_fail_device_build.argtypes = None, [C.c_int]
        lib.sh_debug_held_at_host_build.restype, lib.sh_debug_held_at_host_build.argtypes = C.c_int, []
        lib.sh_debug_p_len.restype, lib.sh_debug_p_len.argtypes = C.c_int64, [C.c_void_p]
        lib.sh_debug_build_verdicts.restype = C.c_int
        lib.sh_debug_build_verdicts.argtypes = [C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] * 3 + [
            C.POINTER(abi.sh_plan_options), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int64]
        self.e = C.c_void_p()
        assert lib.sh_engine_create(0, C.byref(self.e)) == 0

    def close(self):
        self.lib.sh_debug_set_p_limit(0)
        self.lib.sh_debug_fail_device_build(0)
        self.lib.sh_engine_destroy(self.e)

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.sh_last_error(self.e))

    def options(self, **kw):
        opt = abi.sh_plan_options()
        self.lib.sh_plan_options_default(C.byref(opt))
        for k, v in kw.items():
            setattr(opt, k, v)
        return opt

    def verdicts(self, rows, cols, rp, ci, va, **kw):
        host, dev, why = C.c_int32(-9), C.c_int32(-9), C.create_string_buffer(256)
        opt = self.options(plan=2, **kw)
        rc = self.lib.sh_debug_build_verdicts(self.e, rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), C.byref(host), C.byref(dev), why, len(why))
        assert rc == 0, (rc, why.value)
        return host.value, dev.value, why.value.decode()

    def free_bytes(self):
        b = C.c_uint64()
        self.ok(self.lib.sh_engine_synchronize(self.e))
        self.ok(self.lib.sh_engine_max_alloc(self.e, C.byref(b)))
        return b.value

    def upload(self, rows, cols, rp, ci, va, **kw):
        h = C.c_void_p()
        opt = self.options(**kw)
        self.ok(self.lib.sh_csr_upload_ex(self.e, rows, cols, len(ci), _p(rp), _p(ci), _p(va), C.byref(opt), C.byref(h)))
        return Matrix(self, h)

    def vector(self, a):
        h = C.c_void_p()
        a = np.ascontiguousarray(a)
        self.ok(self.lib.sh_vec_alloc(self.e, len(a), C.byref(h)))
        self.ok(self.lib.sh_vec_upload(self.e, h, _p(a), len(a)))
        return h

    def spmv(self, sr, A, x, y, rows):
        """out = alpha (A (x) x) (+) beta y under SCALARS[sr], downloaded."""
        dt = O.elem_dtype(sr)
        a, b = (np.array([v], dt) for v in SCALARS[sr])
        xv, yv, ov = self.vector(x), self.vector(y), self.vector(np.zeros(rows, dt))
        self.ok(self.lib.sh_spmv(self.e, sr, A.h, xv, yv, _p(a), _p(b), ov, None, None))
        out = np.zeros(rows, dt)
        self.ok(self.lib.sh_vec_download(self.e, ov, _p(out), rows))
        for v in (xv, yv, ov):
            self.lib.sh_vec_free(self.e, v)
        return out


class Matrix:
    def __init__(self, tools, h):
        self.t, self.h = tools, h

    def plan(self):
        p = C.c_int32(-1)
        self.t.ok(self.t.lib.sh_csr_plan(self.h, C.byref(p), None))
        return p.value

    def describe(self):
        buf = C.create_string_buffer(256)
        self.t.ok(self.t.lib.sh_csr_describe(self.h, buf, len(buf)))
        return buf.value.decode()

    def layout(self):
        """describe() without the device bytes at its end (footprint() compares those exactly)."""
        return self.describe().split(" device=")[0]

    def footprint(self):
        b = C.c_uint64()
        self.t.ok(self.t.lib.sh_csr_footprint(self.h, C.byref(b)))
        return b.value

    def builder(self):
        w, note = C.c_int32(-1), C.create_string_buffer(256)
        self.t.ok(self.t.lib.sh_csr_builder(self.h, C.byref(w), note, len(note)))
        return ("device" if w.value else "host"), note.value.decode()

    def p_len(self):
        return self.t.lib.sh_debug_p_len(self.h)

    def free(self):
        if self.h is not None:
            self.t.lib.sh_csr_free(self.t.e, self.h)
            self.h = None


@pytest.fixture(scope="module")
def tools():
    t = Tools()
    yield t
    t.close()


@pytest.fixture()
def tl(tools):
    """The tools library with both switches off before and after a test."""
    tools.lib.sh_debug_set_p_limit(0)
    tools.lib.sh_debug_fail_device_build(0)
    yield tools
    tools.lib.sh_debug_set_p_limit(0)
    tools.lib.sh_debug_fail_device_build(0)


def p_limit_matrix():
    rows, cols = 3000, 100_000
    rp, ci, va = random_matrix(np.random.default_rng(301), rows, cols, 12, 3)
    return rows, cols, rp, ci, va


_wanted = {}


def wanted(key, rows, cols, rp, ci, va):
    """The oracle's answers for a matrix, computed once per module: {semiring: (values, x, y, result)}."""
    if key not in _wanted:
        res = {}
        for sr in SEMIRINGS:
            integer = sr in (O.OR_AND_I32, O.MAX_MIN_I32)
            dt = O.elem_dtype(sr)
            vals = va.astype(np.int32) if integer else va
            x = (np.arange(cols) % 3 == 0).astype(np.int32) if integer else (1 + np.arange(cols) % 7).astype(np.float32)
            y = (np.arange(rows) % 5).astype(dt)
            res[sr] = (vals, x, y, O.kernel(sr, rp, ci, vals, x, y, *SCALARS[sr]))
        _wanted[key] = res
    return _wanted[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- (a)
@pytest.mark.parametrize("name", sorted(S.TABLE))
def test_both_builders_give_the_same_verdict(tl, name):
    make, built, why_want = S.TABLE[name]
    rows, cols, rp, ci, va = make()
    host, dev, why = tl.verdicts(rows, cols, rp, ci, va)
    assert (host, dev) == (int(built), int(built)), (host, dev, why)
    if not built:
        assert why_want in why, why


@pytest.mark.parametrize("fold", [1, 0])
def test_both_builders_give_the_same_verdict_at_the_limit_of_p(tl, fold):
    rows, cols, rp, ci, va = p_limit_matrix()
    A = tl.upload(rows, cols, rp, ci, va, plan=2, build=1, fold=fold)
    p_len = A.p_len()
    A.free()
    assert p_len > 0 and p_len % 4 == 0
    tl.lib.sh_debug_set_p_limit(p_len)
    assert tl.verdicts(rows, cols, rp, ci, va, fold=fold)[:2] == (1, 1)
    tl.lib.sh_debug_set_p_limit(p_len - 4)
    host, dev, why = tl.verdicts(rows, cols, rp, ci, va, fold=fold)
    assert (host, dev) == (0, 0) and S.WHY_P in why, (host, dev, why)
    tl.lib.sh_debug_set_p_limit(0)
    assert tl.verdicts(rows, cols, rp, ci, va, fold=fold)[:2] == (1, 1)


# ---- (b)
REFUSED = {
    "light_150_bins": (lambda: S.light_pieces(150), S.WHY_PADDING),
    "heavy_100_rows": (lambda: S.heavy_strips(100), S.WHY_PADDING),
    "p_limit": (p_limit_matrix, S.WHY_P),
}


@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_a_refused_tiled_plan_ends_in_a_working_stream_matrix(tl, name, build):
    """plan = 2 asked, the layout's limits say no: the matrix runs on the CSR-stream plan and says so, sh_csr_builder
    reports the host (nothing was built on the device) with the device builder's reason as its note when that builder
    was the one asked ("Limits of the tiled layout"), the four semirings give the oracle's bits, and the
    matrix holds exactly what a plan = 1 upload holds.  At the limit itself the same matrix is tiled, same bits."""
    make, why_want = REFUSED[name]
    rows, cols, rp, ci, va = make()
    want = wanted(name, rows, cols, rp, ci, va)
    p_len = None
    if name == "p_limit":
        A = tl.upload(rows, cols, rp, ci, va, plan=2, build=build)
        assert A.plan() == 1 and A.describe().startswith("tiled")
        p_len = A.p_len()
        A.free()
        tl.lib.sh_debug_set_p_limit(p_len - 4)
    for sr in SEMIRINGS:
        vals, x, y, ref = want[sr]
        if sr in (O.MIN_PLUS_F32, O.MAX_MIN_I32):
            continue                                   # (the matrix of the semiring in front serves: same value words)
        A = tl.upload(rows, cols, rp, ci, vals, plan=2, build=build)
        B = tl.upload(rows, cols, rp, ci, vals, plan=1, build=build)
        assert A.plan() == 0 and A.describe().startswith("stream"), A.describe()
        assert A.builder() == ("host", why_want if build == 2 else ""), A.builder()
        assert A.describe() == B.describe()
        assert A.footprint() == B.footprint()
        for s2 in (sr, {O.PLUS_TIMES_F32: O.MIN_PLUS_F32, O.OR_AND_I32: O.MAX_MIN_I32}[sr]):
            _, x2, y2, ref2 = want[s2]
            got = tl.spmv(s2, A, x2, y2, rows)
            np.testing.assert_array_equal(bits(got), bits(ref2), err_msg=f"semiring {s2}")
        A.free()
        B.free()
    if p_len is not None:
        tl.lib.sh_debug_set_p_limit(p_len)
        for sr in (O.PLUS_TIMES_F32, O.OR_AND_I32):
            vals = want[sr][0]
            A = tl.upload(rows, cols, rp, ci, vals, plan=2, build=build)
            assert A.plan() == 1 and A.describe().startswith("tiled"), A.describe()
            assert A.builder() == (("device" if build == 2 else "host"), "")
            assert A.p_len() == p_len
            for s2 in (sr, {O.PLUS_TIMES_F32: O.MIN_PLUS_F32, O.OR_AND_I32: O.MAX_MIN_I32}[sr]):
                _, x2, y2, ref2 = want[s2]
                np.testing.assert_array_equal(bits(tl.spmv(s2, A, x2, y2, rows)), bits(ref2), err_msg=f"tiled, semiring {s2}")
            A.free()


# ---- (c)
@pytest.mark.parametrize("build", [1, 2])
def test_more_tiles_than_a_tile_number_holds_uploads_on_the_stream_plan(tl, build):
    rows, cols, rp, ci, va = S.too_many_tiles()
    A = tl.upload(rows, cols, rp, ci, va, plan=2, build=build)
    B = tl.upload(rows, cols, rp, ci, va, plan=1, build=build)
    assert A.plan() == 0 and A.describe().startswith("stream"), A.describe()
    assert A.builder() == ("host", S.WHY_TILES if build == 2 else "")
    assert A.describe() == B.describe() and A.footprint() == B.footprint()
    A.free()
    B.free()


# ---- (d)
def test_a_failed_device_build_step_falls_back_to_the_host_builder(tl):
    """sh_debug_fail_device_build(1): the device builder fails before it has allocated anything; (2): after it has built
    everything.  Either way the matrix is the host-built one (note "injected"), the next upload uses the device builder
    again, and the device holds no more afterwards than the same uploads leave behind without the switch."""
    rows, nnz = 60_000, 1_200_000                      # 30 bins, 201 heavy rows, 2 tiles
    rp, ci, va = H.powerlaw(rows, nnz)
    want = wanted("powerlaw", rows, rows, rp, ci, va)
    up = dict(plan=2, placement_tries=1)

    def sequence(switches):
        """Host-built, then one device-asked upload per switch, then one more; checks them, frees them; returns (free
        device memory before the first upload, after the last free)."""
        before = tl.free_bytes()
        for sr in (O.PLUS_TIMES_F32, O.OR_AND_I32):
            vals = want[sr][0]
            Ah = tl.upload(rows, rows, rp, ci, vals, build=1, **up)
            assert Ah.builder() == ("host", "") and Ah.plan() == 1
            ms = []
            for where in switches:
                tl.lib.sh_debug_fail_device_build(where)
                M = tl.upload(rows, rows, rp, ci, vals, build=2, **up)
                if where:
                    assert M.builder() == ("host", "injected"), M.builder()
                    # released BEFORE the host builder ran (the upload's scope guard frees them at return in any case,
                    # so the free-memory check below cannot see arrays that were merely held too long)
                    assert tl.lib.sh_debug_held_at_host_build() == 0
                else:
                    assert M.builder() == ("device", ""), M.builder()
                ms.append(M)
            last = tl.upload(rows, rows, rp, ci, vals, build=2, **up)   # the switch applied to one call only
            assert last.builder() == ("device", ""), last.builder()
            ms.append(last)
            for M in ms:
                assert M.plan() == 1
                assert M.describe() == Ah.describe()
                assert M.footprint() == Ah.footprint()
            for s2 in (sr, {O.PLUS_TIMES_F32: O.MIN_PLUS_F32, O.OR_AND_I32: O.MAX_MIN_I32}[sr]):
                _, x, y, ref = want[s2]
                for M in [Ah] + ms:
                    np.testing.assert_array_equal(bits(tl.spmv(s2, M, x, y, rows)), bits(ref), err_msg=f"semiring {s2}, {M.builder()}")
            for M in [Ah] + ms:
                M.free()
        return before, tl.free_bytes()

    sequence((0, 0))                                   # (first use: code objects, rocPRIM's and the allocator's pools)
    b0, a0 = sequence((0, 0))
    b1, a1 = sequence((1, 2))
    print(f"free device memory: unswitched {b0} -> {a0}, switched {b1} -> {a1}")
    assert b1 - a1 <= max(b0 - a0, 0), (b0, a0, b1, a1)
