"""sh_color -- sh_color_graph_create / _free / _footprint / _edges / _max_degree and sh_color -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU
needed)."""
import ctypes as C
import os
import re

import numpy as np

import abi_checks
from abi_checks import CSRC, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_color_graph sh_color_graph;"
WANT = {
    "sh_color_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                              "sh_color_graph * *"],
    "sh_color_graph_free": ["sh_engine *", "sh_color_graph *"],
    "sh_color_graph_footprint": ["const sh_color_graph *", "uint64_t *"],
    "sh_color_graph_edges": ["const sh_color_graph *", "int64_t *"],
    "sh_color_graph_max_degree": ["const sh_color_graph *", "int64_t *"],
    "sh_color": ["sh_engine *", "sh_color_graph *", "sh_vec *", "sh_vec *", "int32_t", "uint32_t", "int32_t", "int32_t",
                 "int32_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}
KERNELS = ("gcol_init", "gcol_count", "gcol_ready", "gcol_assign", "gcol_close")


def test_color_entry_points_are_declared_exported_and_bound():
    # sh_color is the first entry point with a uint32_t passed by value (the seed): the shared map learns the type
    abi_checks.CTYPE.setdefault("uint32_t", C.c_uint32)
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "row r storing column c with 0 <= c < rows", "not all zero",
                 "SIMPLE UNDIRECTED", "Self-loops", "PRECEDES", "lexicographically", "prio[v] (signed int32)",
                 "deg[v] when order == 2", "the smaller index first", "the larger mix32(v ^ seed) first",
                 "x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16", "bijection",
                 "no two vertices tie", "natural first-fit", "JP-R", "JP-LF", "smallest-last", "no bound on the colours",
                 "smallest colour >= 0 held by no neighbour that precedes v", "-1 while v is uncoloured",
                 "largest colour plus 1", "longest chain", "chain depth is r", "deterministic", "every comparison is ==",
                 "do not depend on window", "Hasenplaugh", "computed on the spot", "no key array is stored", "one lane",
                 "one wave", "pieces of 2048", "one atomic add per piece", "one atomic decrement", "old value 1",
                 "no restore is needed", "no compare-and-swap", "32-bit mask", "2049 bits", "far end", "32768 bits",
                 "only the first walk decrements", "len / window + 1", "never adjacent", "coloured once", "joins a list once",
                 "no kernel ever waits", "every loop is bounded", "Worst cases", "takes n rounds", "K_n", "beyond the first window",
                 "Measured on an MI355X", "Rule:", "NOT covered", "distance-2 and bipartite", "balancing the classes",
                 "recolouring to fewer colours", "multi-GPU", "row pieces", "C++ harness apps", "incremental updates",
                 "needs 4 * (rows + 1) + 16 * nnz + 8", "32 bytes per edge", "order outside 0..2",
                 "multiple of 64 in [64, 32768]", "max_rounds < 1", "the scalars are checked first", "before any device work",
                 "Freeing NULL is SH_OK", "rows == 0"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go
    assert "GOES_HERE" not in comment


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_color_gpu.py compares sh_color_graph_footprint with is the header's, and its numbers are
    those of color.hip.h: adj_ptr, adj_col (2M words), deg + wait + two work lists (4 words per row), the control block
    and one WlPart (16 bytes) per workgroup; no piece lists."""
    text = " ".join(section_comment(SECTION, stars=False).split())
    assert "4 * (rows + 1) + 16 * rows + 8 * edges + 17408" in text
    code = open(os.path.join(CSRC, "color.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("GCOL_SHORT", "GCOL_PIECE", "GCOL_BATCH", "GCOL_MAX_BLOCKS", "GCOL_CTL_BYTES", "GCOL_WINDOW")}
    assert const["GCOL_CTL_BYTES"] + 16 * const["GCOL_MAX_BLOCKS"] == 17408
    assert (const["GCOL_SHORT"], const["GCOL_PIECE"], const["GCOL_BATCH"], const["GCOL_WINDOW"]) == (8, 2048, 32, 32768)
    assert "WlPiece" not in code and "wl_push_pieces" not in code   # no piece lists


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create), the scalars first, and
    no output is written."""
    lib = abi.load()
    check_create_errors("sh_color_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_color_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_color_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_color_graph_max_degree(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_color_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    kc, rd, cp, cd = C.c_int32(7), C.c_int32(7), C.c_int32(7), C.c_int64(7)
    outs = (C.byref(kc), C.byref(rd), C.byref(cp), C.byref(cd))
    nulls = (None,) * 4

    def call(order=2, seed=0, window=0, max_rounds=10):
        return lib.sh_color(None, None, None, None, order, seed, window, max_rounds, *outs, *nulls)

    for order in (-1, 3):
        assert call(order=order) == abi.SH_EINVAL and "order" in last_error() and "sh_color" in last_error()
    for window in (-64, 1, 32, 63, 65, 96, 32768 + 64, 65536):
        assert call(window=window) == abi.SH_EINVAL and "window" in last_error(), window
    for max_rounds in (0, -5):
        assert call(max_rounds=max_rounds) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert call(order=3, window=1, max_rounds=0) == abi.SH_EINVAL and "order" in last_error()       # the scalars, in order
    assert call(window=1, max_rounds=0) == abi.SH_EINVAL and "window" in last_error()
    for window in (0, 64, 128, 32768):       # every legal scalar: the NULL handles are next
        assert call(window=window, seed=0xFFFFFFFF) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "color", "colors", "rounds", "complete"):
            assert word in last_error()
    assert (kc.value, rd.value, cp.value, cd.value) == (7, 7, 7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("GCOL_KERNELS", "seen_gcol", "truss_peel", "core_peel", "tri_finish", "wcc_jump", "scc_trim",
                        "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    assert "len(seen_gcol) != len(GCOL_KERNELS)" in src and "offenders" in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "color.hip.h" in mk
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "color.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_color: round\"", "create_graph_handle<sh_color_graph>(e, COLOR_CREATE",
                        "COLOR_CREATE = \"sh_color_graph_create\"", "build_symmetric_lists(e, COLOR_CREATE",
                        "struct sh_color_graph : GraphHandle<ColorCtl>", "free_handle(e, g)"):
        assert k in hip, k
    # the colouring handle reaches build_und_edges through the helper it shares with sh_core_graph_create and
    # sh_truss_graph_create, and tests/test_truss_abi.py's counts stay as they are
    assert hip.count("build_und_edges(e, tmp") == 2 and hip.count("build_symmetric_lists(e, \"sh_") == 2
    assert hip.count("build_symmetric_lists(e, ") == 3
    assert "rocprim" not in hip   # rocPRIM stays in plan_gpu.hip
    code = open(os.path.join(CSRC, "color.hip.h")).read()
    for phrase in ("TWO VERTICES OF ONE LIST ARE NEVER ADJACENT", "EVERY VERTEX IS COLOURED ONCE AND JOINS A LIST ONCE",
                   "A LIST OF `rows` PLACES CANNOT OVERFLOW", "NO KERNEL EVER WAITS", "EVERY LOOP IS BOUNDED",
                   "NO RESTORE IS NEEDED", "ONLY THE FIRST WALK DECREMENTS", "Hasenplaugh"):
        assert phrase in code, phrase
    for k in KERNELS + ("gcol_walk", "gcol_mix32", "0x7feb352du", "0x846ca68bu"):
        assert k in code, k
    # the sum and the largest colour go through the shared folds, and the header defines no workgroup fold of its own
    for k in ("wl_block_part<WlMax>(part, looked, most)", "wl_sum_parts<WlMax>(part, nparts)", "wl_block_fold<WlMin>(best)"):
        assert k in code, k
    assert "__shfl_xor" not in code and "_block_part(WlPart" not in code
    assert not re.search(r"__shared__[^;]*\[WL_BS(?: / 64)?\](?!\[)", code)   # (per-wave bitmaps are [WL_BS / 64][words])
    assert "asm" not in code.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in code and "atomicCAS" not in code   # one decrement per preceding neighbour: no retry loop
    assert "wl_expand" not in code.split("#pragma once")[1]   # a sibling traversal, as truss_walk
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/greedy_colors.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_greedy_colors" in open(os.path.join(host, "inc", "sh_host.h")).read()
    assert os.path.exists(os.path.join(host, "src", "greedy_colors.cpp"))


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    k, l, seven = text.index("## 6k."), text.index("## 6l."), text.index("\n## 7")
    assert k < l < seven
    section = text[l:text.index("\n## ", l + 1)]
    assert section.startswith("## 6l. Greedy vertex colouring (`sh_color_graph_create`, `sh_color`)")
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert "**" + part in section, part
    assert "GOES_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_color_graph_create", "color_bench.py", "bench.py --steps 50 --warmup 10", "wl_expand", "a sibling",
                 "natural order on a path", "K_n", "window", "max_degree + 1", "degeneracy + 1", "unmeasured",
                 "synth:grid-2048", "synth:rmat-18", "distance-2", "smallest-last", "make asm"):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.color_graph(" in readme and "eng.greedy_colors(" in readme and "6l" in readme
    assert "color_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "color_bench.py"))
    profiles = [f for f in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"color_\w+\.json", f)]
    assert len(profiles) >= 2


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.color import ColorGraph
    from sparseharness_amd.engine import Engine
    assert callable(Engine.color_graph) and callable(Engine.greedy_colors) and callable(hostlib.greedy_colors)
    assert issubclass(ColorGraph, engine._Graph) and callable(ColorGraph.free) and ColorGraph._c == "sh_color_graph"
    assert not hasattr(engine, "ColorGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    # what tests/test_abi.py checks for the handle classes of engine.py: every C function the class looks up by its
    # prefix is bound with the types it passes
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_color_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in ColorGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64, "max_degree": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_color_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
        assert hasattr(ColorGraph, suffix), suffix
    assert abi.SIGNATURES["sh_color_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.greedy_colors)
    assert list(sig.parameters) == ["self", "G", "color", "prio", "order", "seed", "window", "max_rounds"]
    defaults = {name: sig.parameters[name].default for name in ("prio", "order", "seed", "window", "max_rounds")}
    assert defaults == {"prio": None, "order": 2, "seed": 0, "window": 0, "max_rounds": None}
    sig = inspect.signature(hostlib.greedy_colors)
    assert list(sig.parameters) == ["row_ptr", "col_idx", "val", "order", "seed", "prio"]
    assert [sig.parameters[p].default for p in ("order", "seed", "prio")] == [0, 0, None]
    rp, ci, va = np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 0], np.int32), np.ones(3, np.float32)
    color, colors, depth = hostlib.greedy_colors(rp, ci, va)     # a triangle, stored one way
    assert color.tolist() == [0, 1, 2] and colors == 3 and depth.tolist() == [0, 1, 2]
    color, colors, depth = hostlib.greedy_colors(rp, ci, va, prio=np.array([0, 5, 9], np.int32))
    assert color.tolist() == [2, 1, 0] and colors == 3 and depth.tolist() == [2, 1, 0]
