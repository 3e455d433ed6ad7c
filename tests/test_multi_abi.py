"""sh_spmm and sh_iterate_multi (several vectors per launch) are declared in include/sparseharness_hip.h, exported by
the library and bound in abi.SIGNATURES with the declared argument types.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import check_entry_points, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_spmm": ["sh_engine *", "sh_semiring", "const sh_csr *", "int32_t", "const sh_vec *", "const sh_vec *",
                "const void *", "const void *", "sh_vec *", "uint64_t *"],
    "sh_iterate_multi": ["sh_engine *", "sh_semiring", "const sh_csr *", "int32_t", "sh_vec *", "const sh_vec *", "sh_vec *",
                         "const void *", "const void *", "double", "int32_t", "int32_t *", "int32_t *", "int32_t *",
                         "uint64_t *", "uint64_t *"],
}


def test_multi_vector_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_new_declarations_cite_what_they_extend():
    comment = section_comment("int sh_spmm(")
    for cite in ("inc/harness.h:149-195", "app/sssp.cpp:97-176", "no counterpart"):
        assert cite in comment


def test_argument_errors_need_no_device():
    """NULL arguments come back as SH_EINVAL before anything touches a device."""
    lib = abi.load()
    assert lib.sh_spmm(None, 0, None, 4, None, None, None, None, None, None) == abi.SH_EINVAL
    n = C.c_int32()
    assert lib.sh_iterate_multi(None, 0, None, 4, None, None, None, None, None, 1e-4, 10, C.byref(n), None, None, None,
                                None) == abi.SH_EINVAL


def test_resource_check_covers_the_multi_vector_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    assert "spmm_csr" in src and "spmv_tiled" in src
