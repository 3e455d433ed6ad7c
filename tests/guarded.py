"""Vector operands as views between guard words: what tests/test_hygiene_gpu.py and tests/test_graph_hygiene_gpu.py
share.  Not a test and not a conftest.

A `Guarded` operand is an sh_vec_wrap view into a larger allocation of its own, GUARD words of a chosen guard on either
side, starting at a chosen word offset behind a 256-byte boundary; `read` brings the whole allocation back and asserts
that no guard word changed.  `Dev` is one engine of one library through the C ABI.  After a HIP call that failed (`Dev.ok`
saw SH_EHIP, or `call` an EngineError with that code) nothing more is started on the device by any module that uses the `_not_halted` fixture: `_halt` says why."""
import ctypes as C

import numpy as np
import pytest

from sparseharness_amd import abi

GUARD = 256
DEAD = 0xDEADBEEF
_halt = []   # why the GPU work of the modules that import this ended early (a HIP call that failed)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want, what):
    got, want = bits(got).ravel(), bits(want).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} words differ, first at {bad[:6].tolist()}: got "
                           f"{[hex(v) for v in got[bad[:6]]]} want {[hex(v) for v in want[bad[:6]]]}")


def call(fn, *args, **kw):
    """fn(...) of the Python binding; a failed HIP call ends the GPU work of the calling module (_halt)."""
    from sparseharness_amd.engine import EngineError
    try:
        return fn(*args, **kw)
    except EngineError as err:
        if err.code == abi.SH_EHIP:
            _halt.append(str(err))
        raise


class Dev:
    """One engine of one library through the C ABI: the production library (Tier 1) or the tools library (Tier 2)."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h
        self.mats = {}

    def ok(self, rc):
        msg = (self.lib.sh_last_error(self.h) or b"").decode() if rc else ""
        if rc == abi.SH_EHIP:
            _halt.append(msg)
        assert rc == abi.SH_OK, (rc, msg)

    # ---- matrices, made once per module
    def matrix(self, key, make, **options):
        key = (key, tuple(sorted(options.items())))
        if key not in self.mats:
            rows, cols, rp, ci, va = make()
            opt = abi.sh_plan_options()
            self.lib.sh_plan_options_default(C.byref(opt))
            for k, v in options.items():
                setattr(opt, k, v)
            m = C.c_void_p()
            self.ok(self.lib.sh_csr_upload_ex(self.h, rows, cols, len(ci), vp(rp), vp(ci), vp(va), C.byref(opt), C.byref(m)))
            self.mats[key] = m
        return self.mats[key]

    def describe(self, m):
        buf = C.create_string_buffer(256)
        self.ok(self.lib.sh_csr_describe(m, buf, len(buf)))
        return buf.value.decode()

    def builder(self, m):
        w = C.c_int32(-1)
        self.ok(self.lib.sh_csr_builder(m, C.byref(w), None, 0))
        return "device" if w.value else "host"

    # ---- vectors: always views into a guarded allocation
    def guarded(self, data, offset=0, guard=DEAD):
        return Guarded(self, data, offset, guard)

    def close(self):
        for m in self.mats.values():
            self.lib.sh_csr_free(self.h, m)
        self.mats.clear()


class Guarded:
    """`data` (4-byte elements, any shape) as a wrapped view that starts GUARD + offset words into an allocation of its own
    (256-byte aligned, so the view sits at `offset` words modulo 4), with at least GUARD guard words on either side."""

    def __init__(self, dev, data, offset, guard):
        self.dev, self.guard = dev, guard
        data = np.ascontiguousarray(data)
        self.n, self.at = data.size, GUARD + offset
        host = np.full(self.at + self.n + GUARD, guard, np.uint32)
        host[self.at:self.at + self.n] = bits(data).ravel()
        self.base, self.v = C.c_void_p(), C.c_void_p()
        dev.ok(dev.lib.sh_vec_alloc(dev.h, len(host), C.byref(self.base)))
        dev.ok(dev.lib.sh_vec_upload(dev.h, self.base, vp(host), len(host)))
        ptr = dev.lib.sh_vec_device_ptr(self.base)
        assert ptr % 256 == 0
        dev.ok(dev.lib.sh_vec_wrap(dev.h, C.c_void_p(ptr + 4 * self.at), self.n, C.byref(self.v)))
        self.total = len(host)

    @property
    def h(self):
        """The view's sh_vec: a Guarded goes wherever sparseharness_amd.engine takes a Vec."""
        return self.v

    def read(self, what):
        """The view's words; asserts that every guard word in front of it and behind it still holds the guard."""
        host = np.zeros(self.total, np.uint32)
        self.dev.ok(self.dev.lib.sh_vec_download(self.dev.h, self.base, vp(host), self.total))
        front, behind = host[:self.at], host[self.at + self.n:]
        assert len(front) >= GUARD and len(behind) >= GUARD
        for name, g, first in (("in front of", front, 0), ("behind", behind, self.at + self.n)):
            bad = np.nonzero(g != self.guard)[0]
            assert len(bad) == 0, f"{what}: {len(bad)} guard words {name} the view changed, first at word {(first + bad[:6] - self.at).tolist()} of the view"
        return host[self.at:self.at + self.n].copy()

    def free(self):
        self.dev.lib.sh_vec_free(self.dev.h, self.v)
        self.dev.lib.sh_vec_free(self.dev.h, self.base)


@pytest.fixture(autouse=True)
def _not_halted():
    """After a failed HIP call nothing more of the importing module is started on the device."""
    if _halt:
        pytest.fail("the module's GPU work ended at: " + _halt[0])
