"""sh_spmm and sh_iterate_multi (several vectors per launch) are declared in include/sparseharness_hip.h, exported by
the library and bound in abi.SIGNATURES with the declared argument types.  No compute is called here (no GPU needed)."""
import ctypes as C
import os
import re

from conftest import ROOT
from sparseharness_amd import abi

HEADER = os.path.join(ROOT, "include", "sparseharness_hip.h")

_vp, _i32, _int, _u64p, _i32p = C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
# C parameter type (name stripped, blanks squeezed) -> ctypes type of the binding
CTYPE = {
    "sh_engine *": _vp, "sh_semiring": _int, "const sh_csr *": _vp, "int32_t": _i32, "const sh_vec *": _vp, "sh_vec *": _vp,
    "const void *": _vp, "uint64_t *": _u64p, "int32_t *": _i32p, "double": C.c_double,
}
WANT = {
    "sh_spmm": ["sh_engine *", "sh_semiring", "const sh_csr *", "int32_t", "const sh_vec *", "const sh_vec *",
                "const void *", "const void *", "sh_vec *", "uint64_t *"],
    "sh_iterate_multi": ["sh_engine *", "sh_semiring", "const sh_csr *", "int32_t", "sh_vec *", "const sh_vec *", "sh_vec *",
                         "const void *", "const void *", "double", "int32_t", "int32_t *", "int32_t *", "int32_t *",
                         "uint64_t *", "uint64_t *"],
}


def declared_parameters(name):
    """The parameter types of `name` as the header declares them, or None."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    if not m:
        return None
    types = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        t = re.sub(r"[A-Za-z_0-9]+$", "", p).strip()   # drop the parameter's name
        types.append(re.sub(r"\s*\*", " *", t))
    return types


def test_multi_vector_entry_points_are_declared_exported_and_bound():
    lib = abi.load()
    for name, want in WANT.items():
        assert declared_parameters(name) == want, f"{name}: not declared in the header with the agreed parameters"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in abi.SIGNATURES, f"{name} is not bound in abi.SIGNATURES"
        res, args = abi.SIGNATURES[name]
        assert res is _int
        assert list(args) == [CTYPE[t] for t in want], f"{name}: abi.SIGNATURES disagrees with the header"
    assert lib.sh_abi_version() == 3   # functions were added, no struct changed


def test_new_declarations_cite_what_they_extend():
    text = open(HEADER).read()
    at = text.index("int sh_spmm(")
    comment = text[text.rindex("/* ----", 0, at):at]
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
