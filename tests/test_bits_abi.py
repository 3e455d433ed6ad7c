"""The packed-bit (or,and) entry points -- sh_bits_spmv, sh_bits_iterate, sh_bits_from_column, sh_bits_to_column -- are
declared in include/sparseharness_hip.h, exported by the library and bound in abi.SIGNATURES with the declared argument
types.  No compute is called here (no GPU needed)."""
import ctypes as C
import os
import re

from conftest import ROOT
from sparseharness_amd import abi

HEADER = os.path.join(ROOT, "include", "sparseharness_hip.h")

_vp, _i32, _i64, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_int
_u64p, _i32p, _u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
# C parameter type (name stripped, blanks squeezed) -> ctypes type of the binding
CTYPE = {
    "sh_engine *": _vp, "const sh_csr *": _vp, "int32_t": _i32, "int64_t": _i64, "const sh_vec *": _vp, "sh_vec *": _vp,
    "const void *": _vp, "uint64_t *": _u64p, "int32_t *": _i32p, "uint32_t *": _u32p,
}
WANT = {
    "sh_bits_spmv": ["sh_engine *", "const sh_csr *", "int32_t", "const sh_vec *", "const sh_vec *", "const void *",
                     "const void *", "sh_vec *", "uint64_t *"],
    "sh_bits_iterate": ["sh_engine *", "const sh_csr *", "int32_t", "sh_vec *", "const sh_vec *", "sh_vec *", "const void *",
                        "const void *", "int32_t", "int32_t *", "int32_t *", "int32_t *", "uint32_t *", "uint64_t *",
                        "uint64_t *"],
    "sh_bits_from_column": ["sh_engine *", "const sh_vec *", "int64_t", "int32_t", "int32_t", "sh_vec *"],
    "sh_bits_to_column": ["sh_engine *", "const sh_vec *", "int64_t", "int32_t", "int32_t", "sh_vec *"],
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


def test_packed_bit_entry_points_are_declared_exported_and_bound():
    lib = abi.load()
    for name, want in WANT.items():
        assert declared_parameters(name) == want, f"{name}: not declared in the header with the agreed parameters"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in abi.SIGNATURES, f"{name} is not bound in abi.SIGNATURES"
        res, args = abi.SIGNATURES[name]
        assert res is _int
        assert list(args) == [CTYPE[t] for t in want], f"{name}: abi.SIGNATURES disagrees with the header"
    assert lib.sh_abi_version() == 3   # functions were added, no struct changed


def test_section_comment_cites_what_it_extends():
    text = open(HEADER).read()
    at = text.index("int sh_bits_spmv(")
    comment = text[text.rindex("/* ----", 0, at):at]
    for cite in ("inc/harness.h:149-195", "app/bfs.cpp:94-174", "no counterpart", "NOT covered"):
        assert cite in comment


def last_error():
    return (abi.load().sh_last_error(None) or b"").decode()


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
