"""sh_tri -- sh_tri_graph_create / _free / _footprint / _edges / _max_forward and sh_tri -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU
needed)."""
import ctypes as C
import os
import re

import numpy as np

from abi_checks import check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_tri_graph sh_tri_graph;"
WANT = {
    "sh_tri_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "int32_t", "sh_tri_graph * *"],
    "sh_tri_graph_free": ["sh_engine *", "sh_tri_graph *"],
    "sh_tri_graph_footprint": ["const sh_tri_graph *", "uint64_t *"],
    "sh_tri_graph_edges": ["const sh_tri_graph *", "int64_t *"],
    "sh_tri_graph_max_forward": ["const sh_tri_graph *", "int64_t *"],
    "sh_tri": ["sh_engine *", "sh_tri_graph *", "sh_vec *", "sh_vec *", "uint64_t *", "uint64_t *", "uint64_t *"],
}


def test_tri_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
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
    text = " ".join(section_comment(SECTION, stars=False).split())
    assert "4 * (rows + 1) + 4 * rows + 4 * edges + 33024" in text
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "tri.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1)) for k in ("TRI_MAX_BLOCKS", "TRI_CTL_BYTES")}
    assert const["TRI_CTL_BYTES"] + 2 * 16 * const["TRI_MAX_BLOCKS"] == 33024


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    for order in (0, 1):
        check_create_errors("sh_tri_graph_create", extra_args=(order,))
    rp, ci, va = np.array([0, 1, 3], np.int32), np.array([0, 1, 0], np.int32), np.ones(3, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for order in (-1, 2, 7):   # (all else is fine; and `order` is told before the arrays are looked at)
        for rows in (2, -1):
            h = C.c_void_p(1)
            assert lib.sh_tri_graph_create(None, rows, 3, p(rp), p(ci), p(va), order, C.byref(h)) == abi.SH_EINVAL
            assert "order" in last_error() and "sh_tri_graph_create" in last_error() and not h.value
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
