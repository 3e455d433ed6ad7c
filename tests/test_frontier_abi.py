"""The frontier-driven iteration -- sh_frontier_create / _free / _footprint / _transpose and sh_iterate_frontier -- is
declared in include/sparseharness_hip.h, exported by the library and bound in abi.SIGNATURES with the declared argument
types; argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_frontier_create": ["sh_engine *", "const sh_csr *", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                           "sh_frontier * *"],
    "sh_frontier_free": ["sh_engine *", "sh_frontier *"],
    "sh_frontier_footprint": ["const sh_frontier *", "uint64_t *"],
    "sh_frontier_transpose": ["sh_engine *", "const sh_frontier *", "int32_t *", "int32_t *"],
    "sh_iterate_frontier": ["sh_engine *", "sh_semiring", "const sh_csr *", "sh_frontier *", "sh_vec *", "const sh_vec *",
                            "sh_vec *", "const void *", "const void *", "double", "int32_t", "double", "int32_t *", "int32_t *",
                            "int32_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}


def test_frontier_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_cites_what_it_extends():
    comment = section_comment("typedef struct sh_frontier sh_frontier;")
    for cite in ("app/sssp.cpp:97-176", "app/bfs.cpp:94-174", "inc/harness.h:149-195", "no counterpart", "NOT covered",
                 "SH_PLUS_TIMES_F32", "sh_iterate_multi", "sh_bits_iterate", "row pieces", "multi-GPU", "C++ harness apps"):
        assert cite in comment, cite


def iterate(sr, delta, max_iters):
    it, conv = C.c_int32(), C.c_int32()
    return abi.load().sh_iterate_frontier(None, sr, None, None, None, None, None, None, None, delta, max_iters, -1.0,
                                          C.byref(it), C.byref(conv), None, None, None, None, None)


def test_argument_errors_need_no_device():
    """NULL arguments, the semiring that is out of scope, a delta under which an untouched row could fail the convergence
    test and a cap below one launch come back as SH_EINVAL with a telling message before anything touches a device
    (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    h, b = C.c_void_p(), C.c_uint64()
    assert lib.sh_frontier_create(None, None, 0, None, None, None, C.byref(h)) == abi.SH_EINVAL and not h.value
    assert "NULL" in last_error()
    assert lib.sh_frontier_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_frontier_transpose(None, None, None, None) == abi.SH_EINVAL
    assert "NULL" in last_error()
    assert lib.sh_frontier_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    assert iterate(abi.MIN_PLUS_F32, 1e-4, 10) == abi.SH_EINVAL
    assert "NULL" in last_error()
    assert iterate(abi.PLUS_TIMES_F32, 1e-4, 10) == abi.SH_EINVAL
    assert "SH_PLUS_TIMES_F32" in last_error() and "sh_iterate" in last_error()
    for delta in (0.0, -1.0, float("nan")):
        assert iterate(abi.MIN_PLUS_F32, delta, 10) == abi.SH_EINVAL
        assert "delta" in last_error()
    assert iterate(abi.OR_AND_I32, 0.0, 10) == abi.SH_EINVAL   # (exact comparison: delta is not looked at)
    assert "NULL" in last_error()
    for cap in (0, -3):
        assert iterate(abi.OR_AND_I32, 1e-4, cap) == abi.SH_EINVAL
        assert "max_iters" in last_error()
    assert iterate(7, 1e-4, 10) == abi.SH_EINVAL
    assert "semiring" in last_error()


def test_resource_check_covers_the_frontier_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in ("frontier_mark", "frontier_pull", "frontier_apply", "frontier_detect", "msbfs_csr", "spmm_csr", "spmv_tiled"):
        assert k in src
