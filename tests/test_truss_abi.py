"""sh_truss -- sh_truss_graph_create / _free / _footprint / _edges / _max_degree and sh_truss -- is declared in
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

SECTION = "typedef struct sh_truss_graph sh_truss_graph;"
WANT = {
    "sh_truss_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                              "sh_truss_graph * *"],
    "sh_truss_graph_free": ["sh_engine *", "sh_truss_graph *"],
    "sh_truss_graph_footprint": ["const sh_truss_graph *", "uint64_t *"],
    "sh_truss_graph_edges": ["const sh_truss_graph *", "int64_t *"],
    "sh_truss_graph_max_degree": ["const sh_truss_graph *", "int64_t *"],
    "sh_truss": ["sh_engine *", "sh_truss_graph *", "sh_vec *", "sh_vec *", "sh_vec *", "sh_vec *", "int32_t", "int32_t *",
                 "int32_t *", "int32_t *", "int32_t *", "uint64_t *", "int32_t *", "int64_t *", "int64_t *", "uint64_t *",
                 "uint64_t *"],
}
KERNELS = ("truss_init", "truss_support", "truss_total", "truss_min", "truss_open", "truss_peel", "truss_close")


def test_truss_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "row r storing column c with 0 <= c < rows", "not all zero",
                 "SIMPLE UNDIRECTED", "Self-loops", "e-th smallest pair (u, v) with u < v", "lexicographic",
                 "|N(u) & N(v)|", "three times the triangles", "Cohen", "truss 2", "every edge of K_n has truss n",
                 "0 until the edge is settled", "max_truss", "levels", "sum of min(deg u, deg v)", "deterministic",
                 "stamp", "current", "gone", "alive", "e < e1", "neither is current", "both are current",
                 "one atomic decrement", "old value s + 1", "restores it with one add", "no compare-and-swap",
                 "one lane", "one wave", "pieces of 2048", "one atomic add per piece", "skipped, not walked", "monotone",
                 "Every edge is settled once", "no kernel ever waits", "every loop is bounded",
                 "Worst cases", "128 rounds", "two passes over all edges", "hub", "n^3",
                 "Measured on an MI355X", "Rule:", "NOT covered", "k-truss subgraph extraction", "multi-GPU", "row pieces",
                 "C++ harness apps", "incremental updates", "needs 4 * (rows + 1) + 16 * nnz + 8", "32 bytes per edge",
                 "max_rounds < 0", "before any device work", "Freeing NULL is SH_OK", "rows == 0", "M == 0"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go
    assert "GOES_HERE" not in comment


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_truss_gpu.py compares sh_truss_graph_footprint with is the header's, and its numbers are
    those of truss.hip.h: adj_ptr and deg (a word per row each), adj_col and adj_eid (2M words each), edge_u, edge_v,
    sup, stamp and the two work lists (M words each), the control block and three parts (16 bytes) per workgroup."""
    text = " ".join(section_comment(SECTION, stars=False).split())
    assert "4 * (rows + 1) + 4 * rows + 40 * edges + 51200" in text
    code = open(os.path.join(CSRC, "truss.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("TRUSS_SHORT", "TRUSS_PIECE", "TRUSS_BATCH", "TRUSS_MAX_BLOCKS", "TRUSS_CTL_BYTES")}
    assert const["TRUSS_CTL_BYTES"] + 3 * 16 * const["TRUSS_MAX_BLOCKS"] == 51200
    assert (const["TRUSS_SHORT"], const["TRUSS_PIECE"], const["TRUSS_BATCH"]) == (8, 2048, 32)
    assert 4 * (2 + 2) + 4 * 4 + 4 * 2 == 40   # adj_col + adj_eid, edge_u + edge_v + sup + stamp, two lists


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_truss_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_truss_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_truss_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_truss_graph_max_degree(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_truss_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    mt, lv, rd, cp, tr = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_uint64(7)
    outs = (C.byref(mt), C.byref(lv), C.byref(rd), C.byref(cp), C.byref(tr))
    nulls = (None,) * 5
    assert lib.sh_truss(None, None, None, None, None, None, -1, *outs, *nulls) == abi.SH_EINVAL
    assert "max_rounds" in last_error() and "sh_truss" in last_error()
    assert lib.sh_truss(None, None, None, None, None, None, 10, *outs, *nulls) == abi.SH_EINVAL and "NULL" in last_error()
    for word in ("engine", "graph", "truss"):
        assert word in last_error()
    assert lib.sh_truss(None, None, None, None, None, None, 0, *outs, *nulls) == abi.SH_EINVAL and "NULL" in last_error()
    assert (mt.value, lv.value, rd.value, cp.value, tr.value) == (7, 7, 7, 7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("core_peel", "tri_finish", "wcc_jump", "scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "truss.hip.h" in mk
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "truss.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_truss: round\"", "create_graph_handle<sh_truss_graph>(e, \"sh_truss_graph_create\"",
                        "struct sh_truss_graph : GraphHandle<TrussCtl>", "free_handle(e, g)", "wl_edge_ends", "wl_edge_ids"):
        assert k in hip
    # the truss build reaches build_und_edges through the helper it shares with sh_core_graph_create
    assert hip.count("build_und_edges(e, tmp") == 2 and hip.count("build_symmetric_lists(e, \"sh_") == 2
    assert "rocprim" not in hip   # rocPRIM stays in plan_gpu.hip
    code = open(os.path.join(CSRC, "truss.hip.h")).read()
    for phrase in ("EVERY TRIANGLE COSTS EACH SURVIVING EDGE ONE DECREMENT", "TRANSIENT VALUES BELOW s ARE HARMLESS",
                   "EVERY EDGE IS SETTLED ONCE", "NO KERNEL EVER WAITS", "EVERY LOOP IS BOUNDED", "PEELING IS MONOTONE"):
        assert phrase in code
    assert "asm" not in code.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in code and "atomicCAS" not in code   # one decrement, one restore: no retry loop
    builders = open(os.path.join(CSRC, "worklist.hip.h")).read()
    for k in ("wl_edge_ends", "wl_edge_ids", "wl_both_ways", "wl_forward_lists"):
        assert k in builders
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/truss_numbers.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_truss_numbers" in open(os.path.join(host, "inc", "sh_host.h")).read()


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    a, b, c = text.index("## 6i."), text.index("## 6j."), text.index("## 6k.")
    assert a < b < c
    for lo, hi in ((a, b), (b, c)):   # the sections of sh_tri and sh_core point here
        not_covered = text[text.rindex("Not covered", lo, hi):hi]
        assert "6k" in not_covered and "sh_truss" in not_covered
    section = text[c:text.index("\n## ", c + 1)]
    assert section.startswith("## 6k. k-truss decomposition (`sh_truss_graph_create`, `sh_truss`)")
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert "**" + part in section, part
    assert "GOES_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_truss_graph_create", "truss_bench.py", "bench.py --steps 50 --warmup 10", "wl_expand", "a sibling",
                 "depth of the peeling", "shorter list", "n³"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.truss_graph(" in readme and "eng.truss_numbers(" in readme and "6k" in readme
    assert "truss_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "truss_bench.py"))


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.truss import TrussGraph
    assert callable(Engine.truss_graph) and callable(Engine.truss_numbers) and callable(hostlib.truss_numbers)
    assert issubclass(TrussGraph, engine._Graph) and callable(TrussGraph.free) and TrussGraph._c == "sh_truss_graph"
    # what tests/test_abi.py checks for the handle classes of engine.py: every C function the class looks up by its
    # prefix is bound with the types it passes
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_truss_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in TrussGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64, "max_degree": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_truss_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
        assert hasattr(TrussGraph, suffix), suffix
    assert abi.SIGNATURES["sh_truss_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.truss_numbers)
    assert list(sig.parameters) == ["self", "G", "truss", "support", "edge_u", "edge_v", "max_rounds"]
    for name in ("support", "edge_u", "edge_v", "max_rounds"):
        assert sig.parameters[name].default is None
    rp, ci, va = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), np.ones(3, np.float32)
    eu, ev, sup, truss, m = hostlib.truss_numbers(rp, ci, va)     # a triangle
    assert truss.tolist() == [3, 3, 3] and sup.tolist() == [1, 1, 1] and m == 3
    assert eu.tolist() == [0, 0, 1] and ev.tolist() == [1, 2, 2]
