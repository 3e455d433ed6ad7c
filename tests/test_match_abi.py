"""sh_match -- sh_match_graph_create / _free / _footprint / _edges and sh_match -- is declared in
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

SECTION = "typedef struct sh_match_graph sh_match_graph;"
WANT = {
    "sh_match_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                              "sh_match_graph * *"],
    "sh_match_graph_free": ["sh_engine *", "sh_match_graph *"],
    "sh_match_graph_footprint": ["const sh_match_graph *", "uint64_t *"],
    "sh_match_graph_edges": ["const sh_match_graph *", "int64_t *"],
    "sh_match": ["sh_engine *", "sh_match_graph *", "sh_vec *", "sh_vec *", "sh_vec *", "sh_vec *", "sh_vec *", "int32_t",
                 "uint32_t", "int32_t", "int64_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *",
                 "uint64_t *", "uint64_t *"],
}
KERNELS = ("match_init", "match_bid", "match_take", "match_clear", "match_close")
FOOTPRINT = "8 * rows + 20 * edges + 17408"


def test_match_entry_points_are_declared_exported_and_bound():
    abi_checks.CTYPE.setdefault("uint32_t", C.c_uint32)   # (the seed is passed by value, as sh_color's)
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "SIMPLE UNDIRECTED", "e-th smallest pair u < v",
                 "k(b) = b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000", "parallel entries included",
                 "Nothing is refused", "A stored +0.0 is no edge", "MKEY(e) = hi(e) << 32 | lo(e)",
                 "hi = k(weight[e]) for heavy == 0", "hi = ~k(weight[e]) for heavy == 1", "lo = e when seed == 0",
                 "lo = mix32(e ^ seed) otherwise", "no two keys are equal", "A key may be all ones only for seed != 0",
                 "takes the edges in ascending MKEY and keeps an edge when both its ends are still free",
                 "rows elements are overwritten, no more", "M elements are overwritten, no more",
                 "Every comparison is ==", "Preis 1999", "Hoepman 2004", "Manne and Bisseling 2007",
                 "no compare-and-swap, no retry, and no lane waits for another", "one lane per edge",
                 "M places cannot overflow", "global_atomic_umin_x2", "locally dominant", "The edge tests itself",
                 "neither launch reads what it writes itself", "concurrent stores store the same value",
                 "never bid for again", "first round with kept_r == 0", "by induction over the rounds", "Determinism",
                 "functions of the input, heavy and seed alone", "rounds <= floor(rows / 2) + 1",
                 "attained on a path whose keys ascend along it", "a valid matching, not a maximal one",
                 "good for another call", "Worst cases", "one pair per round in places", "one best word",
                 "Measured on an MI355X", "Rule:", "unmeasured", "NOT covered", "maximum-cardinality or maximum-weight",
                 "bipartite row-column matching", "np.minimum(v, mate)", "continuing a cut-short run", "multi-GPU",
                 "C++ harness apps", "2M <= 2^31 - 256", FOOTPRINT, "max_rounds < 1", "heavy outside {0, 1}",
                 "the scalars are checked first", "before any device work", "Freeing NULL is SH_OK", "rows == 0",
                 "One handle serves any number of calls, one at a time"):
        assert cite in comment, cite
    assert "@" not in comment and "GO_HERE" not in comment   # no placeholder left where the measurements go


def footprint_of(text):
    """The formula the header states, as a function of rows and edges."""
    m = re.search(r"sh_match_graph_footprint: device bytes held = (\d+) \* rows \+ (\d+) \* edges \+ (\d+)\.", text)
    assert m, "the header states no footprint formula for sh_match_graph"
    a, b, c = (int(x) for x in m.groups())
    return lambda rows, edges: a * rows + b * edges + c


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_match_gpu.py compares sh_match_graph_footprint with is the header's, and its numbers are
    those of match.hip.h: best (8 bytes per row), eu, ev, wk and two work lists (4 bytes per edge each), the control
    block and one WlPart (16 bytes) per workgroup."""
    text = " ".join(section_comment(SECTION, stars=False).split())
    f = footprint_of(text)
    import test_match_gpu
    for rows, edges in ((0, 0), (1, 0), (60, 59), (160_000, 319_200)):
        assert f(rows, edges) == test_match_gpu.header_footprint(rows, edges) == 8 * rows + 20 * edges + 17408
    code = open(os.path.join(CSRC, "match.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("MATCH_BATCH", "MATCH_MAX_BLOCKS", "MATCH_CTL_BYTES")}
    assert const["MATCH_CTL_BYTES"] + 16 * const["MATCH_MAX_BLOCKS"] == 17408
    assert const["MATCH_BATCH"] == 32
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "MATCH_CTL_BYTES + MATCH_PART_BYTES == 17408" in hip
    assert "#define SH_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sparseharness_hip.h")).read()


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device, the scalars first, and no output is written."""
    lib = abi.load()
    check_create_errors("sh_match_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_match_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_match_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_match_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    pr, rd, cp = C.c_int64(7), C.c_int32(7), C.c_int32(7)
    outs = (C.byref(pr), C.byref(rd), C.byref(cp))

    def call(heavy=1, seed=1, max_rounds=4096):
        return lib.sh_match(None, None, None, None, None, None, None, heavy, seed, max_rounds, *outs, *(None,) * 5)

    for max_rounds in (0, -5):
        assert call(max_rounds=max_rounds) == abi.SH_EINVAL and "max_rounds" in last_error() and "sh_match" in last_error()
    for heavy in (-1, 2, 7):
        assert call(heavy=heavy) == abi.SH_EINVAL and "heavy" in last_error() and "sh_match" in last_error()
    for heavy, seed, max_rounds in ((0, 0, 1), (1, 1, 4096), (1, 0xFFFFFFFF, 1 << 20)):   # legal scalars: the NULL handles are next
        assert call(heavy, seed, max_rounds) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "mate", "pairs", "rounds", "complete"):
            assert word in last_error()
    assert (pr.value, rd.value, cp.value) == (7, 7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("MATCH_KERNELS", "seen_match", "msf_find", "gcol_assign", "truss_peel"):
        assert k in src
    assert "len(seen_match) != len(MATCH_KERNELS)" in src and "offenders" in src
    assert len(re.search(r"MATCH_KERNELS = \(([^)]*)\)", src).group(1).split(",")) == len(KERNELS)
    assert "match.hip.h" in open(os.path.join(CSRC, "Makefile")).read()
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "match.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_match: round\"", "create_graph_handle<sh_match_graph>(e, MATCH_CREATE",
                        "MATCH_CREATE = \"sh_match_graph_create\"", "struct sh_match_graph : GraphHandle<MatchCtl>"):
        assert k in hip, k
    assert hip.count("int sh_match_graph_free(sh_engine *e, sh_match_graph *g) { return free_handle(e, g); }") == 1
    # the edge list is built once, by the code sh_msf_graph_create uses
    assert hip.count("static int build_weighted_edges(") == 1 and hip.count("build_weighted_edges(e, ") == 2
    assert hip.count("hipLaunchKernelGGL(msf_weights,") == 1
    code = open(os.path.join(CSRC, "match.hip.h")).read()
    for phrase in ("NO TWO KEYS ARE EQUAL", "THE EDGE TESTS ITSELF", "NEITHER LAUNCH READS WHAT IT WRITES ITSELF",
                   "THE RUN FINISHES AT THE FIRST ROUND THAT KEPT NO EDGE", "NO LIST CAN OVERFLOW ON ANY INPUT",
                   "NO KERNEL EVER WAITS", "Preis", "Hoepman", "Manne and Bisseling", "by induction over the rounds"):
        assert phrase in " ".join(code.replace("//", " ").split()), phrase   # (a phrase may run over a comment's line break)
    for k in KERNELS + ("struct MatchCtl", "MatchRec rec[MATCH_BATCH]", "msf_lower", "gcol_mix32", "wl_wave_append",
                        '#include "msf.hip.h"', '#include "color.hip.h"'):
        assert k in code, k
    body = code.split("#pragma once")[1]
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "0x7feb352d" not in body and "fetch_min" not in body          # mix32 and the bid are shared, not copied
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/greedy_matching.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_greedy_matching" in open(os.path.join(host, "inc", "sh_host.h")).read()
    gold = open(os.path.join(host, "src", "greedy_matching.cpp")).read()
    assert "std::sort" in gold and "best" not in gold   # the definition sorts and takes; it simulates no rounds


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m, n, seven = text.index("## 6m."), text.index("## 6n."), text.index("\n## 7")
    assert m < n < seven
    section = text[n:text.index("\n## ", n + 1)]
    assert section.startswith("## 6n. Greedy matching (`sh_match_graph_create`, `sh_match`)")
    for part in ("Layout", "Schedule", "Why it is right", "Worst cases", "Measurements", "Calling rule", "Not covered"):
        assert "**" + part in section, part
    assert "GO_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_match_graph_create", "match_bench.py", "bench.py --steps 50 --warmup 10", "global_atomic_umin_x2",
                 "locally dominant", "floor(rows / 2) + 1", "70 001 leaves", "synth:grid-2048", "synth:rmat-18", "unit",
                 "unmeasured", "hostlib.greedy_matching", "seed = 1", "make asm", FOOTPRINT):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.match_graph(" in readme and "eng.matching(" in readme and "6n" in readme
    assert "match_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "match_bench.py"))
    profiles = [f for f in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"match_\w+\.json", f)]
    assert len(profiles) >= 3


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.match import MatchGraph
    assert callable(Engine.match_graph) and callable(Engine.matching) and callable(hostlib.greedy_matching)
    assert issubclass(MatchGraph, engine._Graph) and callable(MatchGraph.free) and MatchGraph._c == "sh_match_graph"
    assert not hasattr(engine, "MatchGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_match_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in MatchGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_match_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_match_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.matching)
    assert list(sig.parameters) == ["self", "G", "mate", "heavy", "seed", "in_match", "edge_u", "edge_v", "weight", "max_rounds"]
    defaults = {name: p.default for name, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"heavy": 1, "seed": 1, "in_match": None, "edge_u": None, "edge_v": None, "weight": None,
                        "max_rounds": 4096}
    assert list(inspect.signature(hostlib.greedy_matching).parameters) == ["row_ptr", "col_idx", "val", "heavy", "seed"]
    # a path 0 - 1 - 2 - 3 weighing 1, 3, 2: heaviest first takes the middle edge alone, lightest first the two others
    rp, ci = np.array([0, 0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)
    va = np.array([1, 3, 2], np.float32)
    eu, ev, w, chosen, mate, M, pairs = hostlib.greedy_matching(rp, ci, va)
    assert eu.tolist() == [0, 1, 2] and ev.tolist() == [1, 2, 3] and w.view(np.float32).tolist() == [1.0, 3.0, 2.0]
    assert chosen.tolist() == [0, 1, 0] and mate.tolist() == [-1, 2, 1, -1] and (M, pairs) == (3, 1)
    eu, ev, w, chosen, mate, M, pairs = hostlib.greedy_matching(rp, ci, va, heavy=0, seed=0)
    assert chosen.tolist() == [1, 0, 1] and mate.tolist() == [1, 0, 3, 2] and pairs == 2
