"""What the tests/test_*_abi.py files share: reading include/sparseharness_hip.h, the C type -> ctypes map, and the
checks every group of entry points gets.  Each file keeps its own WANT table, the phrases it cites and the argument errors
of its drivers.  No compute is called here (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from sparseharness_amd import abi

HEADER = os.path.join(ROOT, "include", "sparseharness_hip.h")
CSRC = os.path.join(ROOT, "sparseharness_amd", "csrc")

_vp = C.c_void_p
# C parameter type (name stripped, blanks squeezed) -> ctypes type of the binding; handles go by pattern (ctype_of)
CTYPE = {
    "sh_semiring": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double,
    "const void *": _vp, "const int32_t *": _vp,
    "uint64_t *": C.POINTER(C.c_uint64), "int64_t *": C.POINTER(C.c_int64), "int32_t *": C.POINTER(C.c_int32),
    "uint32_t *": C.POINTER(C.c_uint32), "double *": C.POINTER(C.c_double),
}


def ctype_of(t):
    """The ctypes type a parameter declared as `t` is bound with: every handle (sh_engine, sh_csr, sh_vec, sh_*_graph,
    sh_frontier) is opaque, so a pointer to one is a void pointer and a pointer to that pointer an out-parameter."""
    if t in CTYPE:
        return CTYPE[t]
    if re.fullmatch(r"(const )?sh_\w+ \*", t):
        return _vp
    if re.fullmatch(r"sh_\w+ \* \*", t):
        return C.POINTER(_vp)
    raise KeyError(t)


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


def check_entry_points(want):
    """Every function of `want` (name -> declared parameter types) is declared so in the header, exported by the library
    and bound in abi.SIGNATURES with the matching ctypes."""
    lib = abi.load()
    for name, types in want.items():
        assert declared_parameters(name) == types, f"{name}: not declared in the header with the agreed parameters"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in abi.SIGNATURES, f"{name} is not bound in abi.SIGNATURES"
        res, args = abi.SIGNATURES[name]
        assert res is C.c_int
        assert list(args) == [ctype_of(t) for t in types], f"{name}: abi.SIGNATURES disagrees with the header"
    assert lib.sh_abi_version() == 3   # functions were added, no struct changed


def section_comment(anchor, stars=True):
    """The header's section comment in front of `anchor` (a typedef line or the start of a declaration); stars=False:
    without the comment's leading stars, so that a phrase may run over a line break once blanks are squeezed."""
    text = open(HEADER).read()
    at = text.index(anchor)
    comment = text[text.rindex("/* ----", 0, at):at]
    return comment if stars else re.sub(r"\n \*", "\n", comment)


def last_error():
    return (abi.load().sh_last_error(None) or b"").decode()


def check_create_errors(name, extra_args=()):
    """Every argument error of check_host_csr comes back from `name` (a sh_*_graph_create; extra_args: what it takes
    between val and out) with a message that names the argument and the function, before anything touches a device, and
    no handle is written (without an engine the message is the thread's, as for sh_engine_create)."""
    def create(rows, nnz, rp, ci, va, out=True):
        h = C.c_void_p(1)   # (stale: the call has to clear it)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        rc = getattr(abi.load(), name)(None, rows, nnz, p(rp), p(ci), p(va), *extra_args, C.byref(h) if out else None)
        assert not h.value or not out, f"{name} wrote a handle"
        assert name in last_error()
        return rc

    rp = np.array([0, 1, 3], np.int32)
    ci, va = np.array([0, 1, 0], np.int32), np.ones(3, np.float32)
    assert create(-1, 3, rp, ci, va) == abi.SH_EINVAL and "rows" in last_error()
    assert create(2, -3, rp, ci, va) == abi.SH_EINVAL and "nnz" in last_error()
    assert create(2, 3, None, ci, va) == abi.SH_EINVAL and "NULL" in last_error() and "row_ptr" in last_error()
    assert create(2, 3, rp, None, va) == abi.SH_EINVAL and "NULL" in last_error() and "col_idx" in last_error()
    assert create(2, 3, rp, ci, None) == abi.SH_EINVAL and "NULL" in last_error() and "val" in last_error()
    assert create(2, 3, rp, ci, va, out=False) == abi.SH_EINVAL and "NULL" in last_error() and "out" in last_error()
    assert create(2, 3, np.array([1, 1, 3], np.int32), ci, va) == abi.SH_ESHAPE and "row_ptr[0]" in last_error()
    assert create(2, 2, rp, ci, va) == abi.SH_ESHAPE and "row_ptr[rows]" in last_error()
    assert create(2, 3, np.array([0, 4, 3], np.int32), ci, va) == abi.SH_ESHAPE and "decreases" in last_error()
    assert create(2, 3, rp, ci, va) == abi.SH_EINVAL and "NULL" in last_error() and "engine" in last_error()   # (all else is fine)
