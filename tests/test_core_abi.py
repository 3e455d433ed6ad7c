"""sh_core -- sh_core_graph_create / _free / _footprint / _edges / _max_degree and sh_core -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU
needed)."""
import ctypes as C
import os
import re

import numpy as np

from abi_checks import CSRC, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_core_graph sh_core_graph;"
WANT = {
    "sh_core_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                             "sh_core_graph * *"],
    "sh_core_graph_free": ["sh_engine *", "sh_core_graph *"],
    "sh_core_graph_footprint": ["const sh_core_graph *", "uint64_t *"],
    "sh_core_graph_edges": ["const sh_core_graph *", "int64_t *"],
    "sh_core_graph_max_degree": ["const sh_core_graph *", "int64_t *"],
    "sh_core": ["sh_engine *", "sh_core_graph *", "sh_vec *", "sh_vec *", "int32_t", "int32_t", "int32_t *", "int32_t *",
                "int32_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}


def test_core_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("app/scc.cpp:96-176", "inc/harness.h:149-195", "the reference has no counterpart",
                 "row r storing column c with 0 <= c < rows", "not all zero", "SIMPLE UNDIRECTED", "Self-loops",
                 "do not depend on chase", "deterministic", "exactly the vertices whose remaining degree fell to <= k",
                 "informational", "never larger than with chase == 0", "monotone", "one atomic decrement", "old value k + 1",
                 "restores it with one add", "no compare-and-swap", "n / (2 (chase + 1))", "chase * 8", "skipped, not walked",
                 "Every vertex is settled once", "no kernel ever waits", "every loop is bounded",
                 "Worst cases", "127 rounds", "two passes over all vertices", "in pieces",
                 "Measured on an MI355X", "Rule:", "NOT covered", "degeneracy ordering", "k-truss", "multi-GPU", "row pieces",
                 "C++ harness apps", "incremental updates", "needs 4 * (rows + 1) + 16 * nnz + 8", "32 bytes per edge",
                 "chase < 0", "max_rounds < 1", "before any device work", "Freeing NULL is SH_OK", "rows == 0"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go
    assert "MEASUREMENTS_GO_HERE" not in comment


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_core_gpu.py compares sh_core_graph_footprint with is the header's, and its numbers are
    those of core.hip.h: adj_ptr, adj_col (2M words), deg + cur + two work lists (4 words per row), two piece lists of
    2M / (CORE_PIECE / 2) + 1 places of 8 bytes, the control block and two WlParts (16 bytes) per workgroup."""
    text = " ".join(section_comment(SECTION, stars=False).split())
    assert "4 * (rows + 1) + 8 * edges + 16 * rows + 16 * (2 * edges / 1024 + 1) + 34816" in text
    code = open(os.path.join(CSRC, "core.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("CORE_SHORT", "CORE_PIECE", "CORE_BATCH", "CORE_MAX_BLOCKS", "CORE_CTL_BYTES")}
    assert const["CORE_CTL_BYTES"] + 2 * 16 * const["CORE_MAX_BLOCKS"] == 34816
    assert const["CORE_PIECE"] // 2 == 1024 and (const["CORE_SHORT"], const["CORE_PIECE"], const["CORE_BATCH"]) == (8, 2048, 32)
    assert "wl_expand<CORE_SHORT, CORE_PIECE>" in code


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_core_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_core_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_core_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_core_graph_max_degree(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_core_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    d, lv, rd, cp = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int32(7)
    outs = (C.byref(d), C.byref(lv), C.byref(rd), C.byref(cp))
    nulls = (None,) * 6
    assert lib.sh_core(None, None, None, None, -1, 10, *outs, *nulls) == abi.SH_EINVAL
    assert "chase" in last_error() and "sh_core" in last_error()
    assert lib.sh_core(None, None, None, None, 0, 0, *outs, *nulls) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert lib.sh_core(None, None, None, None, 0, -5, *outs, *nulls) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert lib.sh_core(None, None, None, None, 0, 10, *outs, *nulls) == abi.SH_EINVAL and "NULL" in last_error()
    for word in ("engine", "graph", "core"):
        assert word in last_error()
    assert (d.value, lv.value, rd.value, cp.value) == (7, 7, 7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    kernels = ("core_init", "core_min", "core_open", "core_peel", "core_close")
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in kernels + ("tri_finish", "wcc_jump", "scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "core.hip.h" in mk
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "core.hip.h"' in hip
    # (sh_core_graph_create checks its host arrays through the helper every sh_*_graph_create goes through)
    for k in kernels + ("run_batches(e, \"sh_core: round\"", "create_graph_handle<sh_core_graph>(e, \"sh_core_graph_create\"",
                        "build_und_edges"):
        assert k in hip
    helper = hip[hip.index("static int create_graph_handle("):]
    assert "check_host_csr(e, fn, rows, nnz, row_ptr, col_idx, val, out)" in helper[:helper.index("\n}\n")]
    assert hip.count("build_und_edges(e, tmp") == 2   # sh_tri_graph_create and sh_core_graph_create share the first half
    code = open(os.path.join(CSRC, "core.hip.h")).read()
    for phrase in ("NO KERNEL EVER WAITS", "EVERY VERTEX IS SETTLED ONCE", "EVERY LOOP IS BOUNDED", "PEELING IS MONOTONE",
                   "TRANSIENT VALUES BELOW k ARE HARMLESS"):
        assert phrase in code
    assert "asm" not in code.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in code and "atomicCAS" not in code   # one decrement, one restore: no retry loop
    builders = open(os.path.join(CSRC, "worklist.hip.h")).read()
    for k in ("wl_und_flag", "wl_und_keys", "wl_run_heads", "wl_und_degrees", "wl_both_ways", "wl_forward_lists", "wl_max_len"):
        assert k in builders and k in hip
    assert "rocprim" not in hip   # rocPRIM stays in plan_gpu.hip
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/core_numbers.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_core_numbers" in open(os.path.join(host, "inc", "sh_host.h")).read()


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    a, b = text.index("## 6i."), text.index("## 6j.")
    assert a < b
    not_covered = text[text.rindex("Not covered", a, b):b]
    assert "6j" in not_covered and "sh_core" in not_covered
    section = text[b:text.index("\n## ", b + 1)]
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert "**" + part in section, part
    assert "MEASUREMENTS_GO_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_core_graph_create", "chase", "core_bench.py", "bench.py --steps 50 --warmup 10"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.core_graph(" in readme and "eng.core_numbers(" in readme and "6j" in readme
    assert "core_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "core_bench.py"))


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import hostlib
    from sparseharness_amd.engine import CoreGraph, Engine
    assert callable(Engine.core_graph) and callable(Engine.core_numbers) and callable(hostlib.core_numbers)
    for attr in ("edges", "max_degree", "footprint"):
        assert hasattr(CoreGraph, attr)
    assert callable(CoreGraph.free)
    sig = inspect.signature(Engine.core_numbers)
    assert sig.parameters["deg"].default is None and sig.parameters["max_rounds"].default is None
    assert isinstance(sig.parameters["chase"].default, int) and sig.parameters["chase"].default >= 0
    rp, ci, va = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), np.ones(3, np.float32)
    core, deg, m = hostlib.core_numbers(rp, ci, va)     # a triangle
    assert core.tolist() == [2, 2, 2] and deg.tolist() == [2, 2, 2] and m == 3
