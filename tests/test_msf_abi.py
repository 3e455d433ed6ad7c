"""sh_msf -- sh_msf_graph_create / _free / _footprint / _edges and sh_msf -- is declared in include/sparseharness_hip.h
with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the declared argument types;
argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from abi_checks import CSRC, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_msf_graph sh_msf_graph;"
WANT = {
    "sh_msf_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_msf_graph * *"],
    "sh_msf_graph_free": ["sh_engine *", "sh_msf_graph *"],
    "sh_msf_graph_footprint": ["const sh_msf_graph *", "uint64_t *"],
    "sh_msf_graph_edges": ["const sh_msf_graph *", "int64_t *"],
    "sh_msf": ["sh_engine *", "sh_msf_graph *", "sh_vec *", "sh_vec *", "sh_vec *", "sh_vec *", "sh_vec *", "int32_t",
               "int64_t *", "int64_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "int64_t *",
               "uint64_t *", "uint64_t *"],
}
KERNELS = ("msf_weights", "msf_init", "msf_find", "msf_pick", "msf_link", "msf_jump", "msf_close", "msf_top", "msf_label")


def test_msf_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "row r storing column c with 0 <= c < rows", "not all zero",
                 "SIMPLE UNDIRECTED", "Self-loops, stored zeros and columns outside the matrix change nothing",
                 "e-th smallest pair u < v", "total order of their bit patterns",
                 "k(b) = b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000",
                 "-NaN < -inf < ... < -0.0 < denormals < ... < +inf < +NaN", "Nothing is refused", "A stored +0.0 is no edge",
                 "the smallest, by k, over all counting entries (u, v) and (v, u), parallel entries included",
                 "KEY(e) = k(weight[e]) << 32 | e", "No two keys are equal", "unique minimum spanning forest",
                 "Kruskal's algorithm returns when it takes the edges in ascending KEY", "M elements are overwritten, no more",
                 "largest vertex index of v's component", "sh_wcc's comp on the same arrays", "the 32 bits of the chosen entry",
                 "*tree_edges = rows - *components", "comp[v] == v", "Every comparison is ==",
                 "does not depend on the schedule or the run", "Boruvka 1926", "Vineet, Harish, Patidar and Narayanan",
                 "no compare-and-swap, no retry, and no lane waits for another", "every tree is a star",
                 "an edge of a flat list", "no long rows and no pieces", "wave-aggregated push", "M places cannot overflow",
                 "global_atomic_umin_x2", "never suppresses a needed one", "the smaller index hooks and the larger stays a root",
                 "pick reads p and writes only to and in_msf", "must not read a word that the same launch writes",
                 "any order of the lanes", "ceil(d / (MSF_JUMPS + 1))", "17^8 >= 2^31", "static_assert",
                 "finishes when find kept no edge", "top lives in best's memory", "the cut property",
                 "every cycle has length 2", "Pointers never leave a component", "Determinism",
                 "functions of the input alone", "floor(log2(rows)) + 1", "max_rounds = 33 can never cut a run short",
                 "every one of which belongs to the forest", "comp is -1 everywhere", "good for another call",
                 "Worst cases", "M log(rows)", "one best word", "the loads still meet on one line",
                 "however short its list is", "Measured on an MI355X", "Rule:", "unmeasured", "NOT covered",
                 "weight[in_msf == 1].astype(float64).sum()", "negate the values", "parent pointers from a chosen root",
                 "multi-GPU", "row pieces", "C++ harness apps", "incremental updates", "2M <= 2^31 - 256",
                 "16 * rows + 20 * edges + 33792", "max_rounds < 1", "the scalars are checked first",
                 "before any device work", "Freeing NULL is SH_OK", "rows == 0",
                 "One handle serves any number of calls, one at a time"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go
    assert "GOES_HERE" not in comment


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_msf_gpu.py compares sh_msf_graph_footprint with is the header's, and its numbers are those
    of msf.hip.h: p and to (4 bytes per row), best (8), eu, ev, wk and two work lists (4 bytes per edge each), the control
    block and two WlParts (16 bytes) per workgroup; and the sweeps make a star of any chain."""
    text = " ".join(section_comment(SECTION, stars=False).split())
    assert "16 * rows + 20 * edges + 33792" in text
    code = open(os.path.join(CSRC, "msf.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("MSF_BATCH", "MSF_MAX_BLOCKS", "MSF_CTL_BYTES", "MSF_JUMPS", "MSF_SWEEPS")}
    assert const["MSF_CTL_BYTES"] + 2 * 16 * const["MSF_MAX_BLOCKS"] == 33792
    assert const["MSF_BATCH"] == 32
    assert (const["MSF_JUMPS"] + 1) ** const["MSF_SWEEPS"] >= 2 ** 31
    assert "static_assert(msf_pow(MSF_JUMPS + 1, MSF_SWEEPS) >= (1ull << 31)" in code
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "MSF_CTL_BYTES + 2 * MSF_PART_BYTES == 33792" in hip
    assert "#define SH_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sparseharness_hip.h")).read()


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create), the scalar first, and no
    output is written."""
    lib = abi.load()
    check_create_errors("sh_msf_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_msf_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_msf_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_msf_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    te, cc, rd, cp = C.c_int64(7), C.c_int64(7), C.c_int32(7), C.c_int32(7)
    outs = (C.byref(te), C.byref(cc), C.byref(rd), C.byref(cp))

    def call(max_rounds=33):
        return lib.sh_msf(None, None, None, None, None, None, None, max_rounds, *outs, *(None,) * 6)

    for max_rounds in (0, -5):
        assert call(max_rounds) == abi.SH_EINVAL and "max_rounds" in last_error() and "sh_msf" in last_error()
    for max_rounds in (1, 33, 1 << 20):   # every legal scalar: the NULL handles are next
        assert call(max_rounds) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "in_msf", "tree_edges", "components", "rounds", "complete"):
            assert word in last_error()
    assert (te.value, cc.value, rd.value, cp.value) == (7, 7, 7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("MSF_KERNELS", "seen_msf", "gcol_assign", "truss_peel", "core_peel", "tri_finish", "wcc_jump",
                        "scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    assert "len(seen_msf) != len(MSF_KERNELS)" in src and "offenders" in src
    assert len(re.search(r"MSF_KERNELS = \(([^)]*)\)", src).group(1).split(",")) == len(KERNELS)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "msf.hip.h" in mk
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "msf.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_msf: round\"", "create_graph_handle<sh_msf_graph>(e, MSF_CREATE",
                        "MSF_CREATE = \"sh_msf_graph_create\"", "build_und_edges(e, build", "wl_edge_ends",
                        "struct sh_msf_graph : GraphHandle<MsfCtl>", "free_handle(e, g)"):
        assert k in hip, k
    assert hip.count("int sh_msf_graph_free(sh_engine *e, sh_msf_graph *g) { return free_handle(e, g); }") == 1
    assert "rocprim" not in hip   # rocPRIM stays in plan_gpu.hip
    code = open(os.path.join(CSRC, "msf.hip.h")).read()
    for phrase in ("NO TWO KEYS ARE EQUAL", "AT THE START OF EVERY ROUND EVERY TREE IS A STAR",
                   "PICK READS p AND WRITES ONLY to AND in_msf", "ANY ORDER OF THE LANES", "FIND KEPT NO EDGE",
                   "NO LIST CAN OVERFLOW ON ANY INPUT", "NO KERNEL EVER WAITS", "Vineet", "1926"):
        assert phrase in " ".join(code.replace("//", " ").split()), phrase   # (a phrase may run over a comment's line break)
    for k in KERNELS + ("struct MsfCtl", "MsfRec rec[MSF_BATCH]", "__hip_atomic_fetch_min", "wl_wave_append"):
        assert k in code, k
    body = code.split("#pragma once")[1]
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "wl_expand" not in body and "WlPiece" not in body          # a flat list: no long rows, no pieces
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/msf_edges.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_msf_edges" in open(os.path.join(host, "inc", "sh_host.h")).read()
    assert os.path.exists(os.path.join(host, "src", "msf_edges.cpp"))


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    l, m, seven = text.index("## 6l."), text.index("## 6m."), text.index("\n## 7")
    assert l < m < seven
    section = text[m:text.index("\n## ", m + 1)]
    assert section.startswith("## 6m. Minimum spanning forest (`sh_msf_graph_create`, `sh_msf`)")
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert "**" + part in section, part
    assert "GOES_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_msf_graph_create", "msf_bench.py", "bench.py --steps 50 --warmup 10", "global_atomic_umin_x2",
                 "17^8", "ceil(d / 17)", "hub of 70 001 leaves", "synth:grid-2048", "synth:rmat-18", "unit", "unmeasured",
                 "hostlib.msf_edges", "sh_wcc", "make asm"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.msf_graph(" in readme and "eng.spanning_forest(" in readme and "6m" in readme
    assert "msf_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "msf_bench.py"))
    profiles = [f for f in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"msf_\w+\.json", f)]
    assert len(profiles) >= 3


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.msf import MsfGraph
    assert callable(Engine.msf_graph) and callable(Engine.spanning_forest) and callable(hostlib.msf_edges)
    assert issubclass(MsfGraph, engine._Graph) and callable(MsfGraph.free) and MsfGraph._c == "sh_msf_graph"
    assert not hasattr(engine, "MsfGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    # what tests/test_abi.py checks for the handle classes of engine.py: every C function the class looks up by its
    # prefix is bound with the types it passes
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_msf_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in MsfGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_msf_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_msf_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.spanning_forest)
    assert list(sig.parameters) == ["self", "G", "in_msf", "comp", "edge_u", "edge_v", "weight", "max_rounds"]
    defaults = {name: sig.parameters[name].default for name in ("comp", "edge_u", "edge_v", "weight", "max_rounds")}
    assert defaults == {"comp": None, "edge_u": None, "edge_v": None, "weight": None, "max_rounds": 33}
    assert list(inspect.signature(hostlib.msf_edges).parameters) == ["row_ptr", "col_idx", "val"]
    rp, ci = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32)
    eu, ev, w, msf, comp, M, components = hostlib.msf_edges(rp, ci, np.array([3, 1, 2], np.float32))   # a triangle
    assert eu.tolist() == [0, 0, 1] and ev.tolist() == [1, 2, 2] and w.view(np.float32).tolist() == [3.0, 2.0, 1.0]
    assert msf.tolist() == [0, 1, 1] and comp.tolist() == [2, 2, 2] and (M, components) == (3, 1)
