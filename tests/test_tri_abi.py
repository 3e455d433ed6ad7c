"""sh_tri -- sh_tri_graph_create / _free / _footprint / _edges / _max_forward and sh_tri -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU
needed)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from sparseharness_amd import abi

HEADER = os.path.join(ROOT, "include", "sparseharness_hip.h")

_vp, _i32, _i64, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_int
_pp = C.POINTER(C.c_void_p)
_u64p, _i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
# C parameter type (name stripped, blanks squeezed) -> ctypes type of the binding
CTYPE = {
    "sh_engine *": _vp, "sh_tri_graph *": _vp, "const sh_tri_graph *": _vp, "sh_tri_graph * *": _pp,
    "int32_t": _i32, "int64_t": _i64, "sh_vec *": _vp, "const void *": _vp, "const int32_t *": _vp,
    "uint64_t *": _u64p, "int64_t *": _i64p,
}
WANT = {
    "sh_tri_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "int32_t", "sh_tri_graph * *"],
    "sh_tri_graph_free": ["sh_engine *", "sh_tri_graph *"],
    "sh_tri_graph_footprint": ["const sh_tri_graph *", "uint64_t *"],
    "sh_tri_graph_edges": ["const sh_tri_graph *", "int64_t *"],
    "sh_tri_graph_max_forward": ["const sh_tri_graph *", "int64_t *"],
    "sh_tri": ["sh_engine *", "sh_tri_graph *", "sh_vec *", "sh_vec *", "uint64_t *", "uint64_t *", "uint64_t *"],
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


def test_tri_entry_points_are_declared_exported_and_bound():
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
    at = text.index("typedef struct sh_tri_graph sh_tri_graph;")
    return re.sub(r"\n \*", "\n", text[text.rindex("/* ----", 0, at):at])   # (without the comment's leading stars)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment().split())
    for cite in ("app/scc.cpp:96-176", "inc/harness.h:149-195", "the reference has no counterpart",
                 "row r storing column c with 0 <= c < rows", "not all zero", "SIMPLE UNDIRECTED", "Self-loops", "unsigned 64-bit",
                 "does not depend on", "order = 0", "order = 1", "at most sqrt(2M)", "degree >= deg(v) >= |N+(v)|",
                 "found once", "no host loop", "chunks of at most 2048", "No kernel ever waits", "bounded by a list length",
                 "Measured on an MI355X", "Rule:", "NOT covered", "per-edge support", "k-truss", "multi-GPU", "row pieces",
                 "C++ harness apps", "incremental updates", "8-byte aligned", "high word", "untested", "Worst cases",
                 "needs 4 * (rows + 1) + 16 * nnz"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go
    assert "MEASUREMENTS_GO_HERE" not in comment


def test_wcc_design_section_points_here():
    """Triangle counting is what DESIGN.md 6h's "Not covered" now points to 6i for."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    a, b = text.index("## 6h."), text.index("## 6i.")
    assert a < b
    not_covered = text[text.rindex("Not covered", a, b):b]
    assert "6i" in not_covered and "sh_tri" in not_covered
    section = text[b:text.index("\n## ", b + 1)]
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert part in section, part


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_tri_gpu.py compares sh_tri_graph_footprint with is the header's."""
    text = " ".join(section_comment().split())
    assert "4 * (rows + 1) + 4 * rows + 4 * edges + 33024" in text
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "tri.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1)) for k in ("TRI_MAX_BLOCKS", "TRI_CTL_BYTES")}
    assert const["TRI_CTL_BYTES"] + 2 * 16 * const["TRI_MAX_BLOCKS"] == 33024


def last_error():
    return (abi.load().sh_last_error(None) or b"").decode()


def create(rows, nnz, rp, ci=None, va=None, out=True, order=1):
    h = C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = abi.load().sh_tri_graph_create(None, rows, nnz, p(rp), p(ci), p(va), order, C.byref(h) if out else None)
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
    for order in (-1, 2, 7):
        assert create(2, 3, rp, ci, va, order=order) == abi.SH_EINVAL and "order" in last_error()
    for order in (0, 1):
        assert create(2, 3, rp, ci, va, order=order) == abi.SH_EINVAL and "NULL" in last_error() and "engine" in last_error()
    assert "sh_tri_graph_create" in last_error()   # (all else was fine)
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_tri_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_tri_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_tri_graph_max_forward(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_tri_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    t = C.c_uint64()
    assert lib.sh_tri(None, None, None, None, C.byref(t), None, None) == abi.SH_EINVAL and "NULL" in last_error()
    assert "graph" in last_error()


def test_resource_check_covers_the_tri_kernels():
    kernels = ("tri_count_light", "tri_count_heavy", "tri_finish")
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in kernels + ("wcc_jump", "scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "tri.hip.h" in mk
    hip = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "engine.hip")).read()
    assert '#include "tri.hip.h"' in hip
    for k in kernels:
        assert k in hip
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "tri.hip.h")).read()
    for phrase in ("NO KERNEL EVER WAITS", "EVERY TRIANGLE IS FOUND ONCE", "EVERY LOOP IS BOUNDED"):
        assert phrase in code
    assert "asm" not in code.replace("amdgcn", "")   # plain C++ and builtins only
    builders = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "worklist.hip.h")).read()
    for k in ("wl_und_flag", "wl_und_keys", "wl_run_heads", "wl_und_degrees", "wl_orient", "wl_forward_lists"):
        assert k in builders and k in hip
    plan = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "plan_gpu.hip")).read()
    assert "device_sort_keys_u64" in plan and "rocprim" not in hip   # rocPRIM stays in plan_gpu.hip


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import hostlib
    from sparseharness_amd.engine import Engine, TriGraph
    assert callable(Engine.tri_graph) and callable(Engine.triangles) and callable(hostlib.triangle_counts)
    for attr in ("edges", "max_forward", "footprint"):
        assert hasattr(TriGraph, attr)
    assert callable(TriGraph.free)
    assert inspect.signature(Engine.tri_graph).parameters["order"].default == 1
    sig = inspect.signature(Engine.triangles)
    assert sig.parameters["tri"].default is None and sig.parameters["deg"].default is None
