"""The packed-bit (or,and) entry points -- sh_bits_spmv, sh_bits_iterate, sh_bits_from_column, sh_bits_to_column -- are
declared in include/sparseharness_hip.h, exported by the library and bound in abi.SIGNATURES with the declared argument
types.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_bits_spmv": ["sh_engine *", "const sh_csr *", "int32_t", "const sh_vec *", "const sh_vec *", "const void *",
                     "const void *", "sh_vec *", "uint64_t *"],
    "sh_bits_iterate": ["sh_engine *", "const sh_csr *", "int32_t", "sh_vec *", "const sh_vec *", "sh_vec *", "const void *",
                        "const void *", "int32_t", "int32_t *", "int32_t *", "int32_t *", "uint32_t *", "uint64_t *",
                        "uint64_t *"],
    "sh_bits_from_column": ["sh_engine *", "const sh_vec *", "int64_t", "int32_t", "int32_t", "sh_vec *"],
    "sh_bits_to_column": ["sh_engine *", "const sh_vec *", "int64_t", "int32_t", "int32_t", "sh_vec *"],
}


def test_packed_bit_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_cites_what_it_extends():
    comment = section_comment("int sh_bits_spmv(")
    for cite in ("inc/harness.h:149-195", "app/bfs.cpp:94-174", "no counterpart", "NOT covered"):
        assert cite in comment


def test_argument_errors_need_no_device():
    """NULL arguments and a `words` / `source` the kernels do not serve come back as SH_EINVAL before anything touches a
    device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    n = C.c_int32()
    its, conv = (C.c_int32 * 256)(), (C.c_int32 * 256)()
    assert lib.sh_bits_spmv(None, None, 1, None, None, None, None, None, None) == abi.SH_EINVAL
    assert "NULL" in last_error()
    assert lib.sh_bits_iterate(None, None, 1, None, None, None, None, None, 10, C.byref(n), its, conv, None, None,
                               None) == abi.SH_EINVAL
    assert "NULL" in last_error()
    assert lib.sh_bits_from_column(None, None, 4, 1, 0, None) == abi.SH_EINVAL
    assert lib.sh_bits_to_column(None, None, 4, 1, 0, None) == abi.SH_EINVAL
    for words in (3, 0, 16, -1):
        assert lib.sh_bits_spmv(None, None, words, None, None, None, None, None, None) == abi.SH_EINVAL
        assert "words" in last_error()
        assert lib.sh_bits_iterate(None, None, words, None, None, None, None, None, 10, C.byref(n), its, conv, None, None,
                                   None) == abi.SH_EINVAL
        assert "words" in last_error()
        assert lib.sh_bits_from_column(None, None, 4, words, 0, None) == abi.SH_EINVAL
        assert "words" in last_error()
        assert lib.sh_bits_to_column(None, None, 4, words, 0, None) == abi.SH_EINVAL
        assert "words" in last_error()
    for words, source in ((1, 32), (1, -1), (8, 256)):   # source outside [0, 32 * words)
        assert lib.sh_bits_to_column(None, None, 4, words, source, None) == abi.SH_EINVAL
        assert "source" in last_error()
        assert lib.sh_bits_from_column(None, None, 4, words, source, None) == abi.SH_EINVAL
        assert "source" in last_error()


def test_resource_check_covers_the_packed_bit_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    assert "msbfs_csr" in src and "msbfs_long" in src and "spmm_csr" in src and "spmv_tiled" in src
