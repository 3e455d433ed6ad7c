"""sh_wcc -- sh_wcc_graph_create / _free / _footprint / _edges and sh_wcc -- is declared in include/sparseharness_hip.h
with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the declared argument types;
argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from sparseharness_amd import abi

HEADER = os.path.join(ROOT, "include", "sparseharness_hip.h")

_vp, _i32, _i64, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_int
_pp = C.POINTER(C.c_void_p)
_u64p, _i32p, _i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
# C parameter type (name stripped, blanks squeezed) -> ctypes type of the binding
CTYPE = {
    "sh_engine *": _vp, "sh_wcc_graph *": _vp, "const sh_wcc_graph *": _vp, "sh_wcc_graph * *": _pp,
    "int32_t": _i32, "int64_t": _i64, "sh_vec *": _vp, "const void *": _vp, "const int32_t *": _vp,
    "uint64_t *": _u64p, "int32_t *": _i32p, "int64_t *": _i64p,
}
WANT = {
    "sh_wcc_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_wcc_graph * *"],
    "sh_wcc_graph_free": ["sh_engine *", "sh_wcc_graph *"],
    "sh_wcc_graph_footprint": ["const sh_wcc_graph *", "uint64_t *"],
    "sh_wcc_graph_edges": ["const sh_wcc_graph *", "int64_t *"],
    "sh_wcc": ["sh_engine *", "sh_wcc_graph *", "sh_vec *", "int32_t", "int32_t", "int64_t *", "int64_t *", "int32_t *",
               "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
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


def test_wcc_entry_points_are_declared_exported_and_bound():
    lib = abi.load()
    for name, want in WANT.items():
        assert declared_parameters(name) == want, f"{name}: not declared in the header with the agreed parameters"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in abi.SIGNATURES, f"{name} is not bound in abi.SIGNATURES"
        res, args = abi.SIGNATURES[name]
        assert res is _int
        assert list(args) == [CTYPE[t] for t in want], f"{name}: abi.SIGNATURES disagrees with the header"
    assert lib.sh_abi_version() == 3   # functions were added, no struct changed


def section_comment():
    text = open(HEADER).read()
    at = text.index("typedef struct sh_wcc_graph sh_wcc_graph;")
    return text[text.rindex("/* ----", 0, at):at]


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = section_comment()
    for cite in ("row r storing column c with 0 <= c < rows", "not all zero", "direction is ignored", "largest", "does not depend on",
                 "trees only", "No kernel ever waits", "Measured on an MI355X", "Rule:", "NOT covered", "multi-GPU", "row pieces",
                 "C++ harness apps", "component sizes", "histogram", "incremental updates", "max_rounds", "sample"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go


def test_scc_section_points_here():
    """Weakly connected components are no longer among what sh_scc's section lists as not covered without a pointer."""
    text = open(HEADER).read()
    at = text.index("typedef struct sh_scc_graph sh_scc_graph;")
    comment = text[text.rindex("/* ----", 0, at):at]
    assert "sh_wcc" in comment and "6h" in comment


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_wcc_gpu.py compares sh_wcc_graph_footprint with is the header's."""
    text = " ".join(section_comment().split())
    assert "8 * (rows + 1) + 8 * edges + 8 * rows + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 34816" in text


def last_error():
    return (abi.load().sh_last_error(None) or b"").decode()


def wcc(sample, max_rounds):
    k, s, r, c = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
    return abi.load().sh_wcc(None, None, None, sample, max_rounds, C.byref(k), C.byref(s), C.byref(r), C.byref(c),
                             None, None, None, None, None, None)


def create(rows, nnz, rp, ci=None, va=None, out=True):
    h = C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = abi.load().sh_wcc_graph_create(None, rows, nnz, p(rp), p(ci), p(va), C.byref(h) if out else None)
    assert not h.value
    return rc


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
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
    assert "sh_wcc_graph_create" in last_error()
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_wcc_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_wcc_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_wcc_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    for s in (-1, -7):
        assert wcc(s, 10) == abi.SH_EINVAL and "sample" in last_error()
    for cap in (0, -3):
        assert wcc(2, cap) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert wcc(2, 10) == abi.SH_EINVAL and "NULL" in last_error() and "comp" in last_error()
    assert wcc(0, 1) == abi.SH_EINVAL and "NULL" in last_error()   # (sample = 0 and max_rounds = 1 are legal)


def test_resource_check_covers_the_wcc_kernels():
    kernels = ("wcc_init", "wcc_sample", "wcc_compact", "wcc_full", "wcc_jump", "wcc_decide", "wcc_label")
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in kernels + ("scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "wcc.hip.h" in mk
    hip = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "engine.hip")).read()
    assert '#include "wcc.hip.h"' in hip
    for k in kernels:
        assert k in hip
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "wcc.hip.h")).read()
    for phrase in ("TREES ONLY EVER MERGE", "NO LIST CAN OVERFLOW", "NO KERNEL EVER WAITS"):
        assert phrase in code


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import hostlib
    from sparseharness_amd.engine import Engine, WccGraph
    assert callable(Engine.wcc_graph) and callable(Engine.wcc) and callable(hostlib.wcc_labels)
    assert hasattr(WccGraph, "edges") and hasattr(WccGraph, "footprint") and callable(WccGraph.free)
    sig = inspect.signature(Engine.wcc)
    assert sig.parameters["sample"].default == 2 and sig.parameters["max_rounds"].default == 1 << 20
