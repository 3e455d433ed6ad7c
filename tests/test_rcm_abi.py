"""sh_rcm -- sh_rcm_graph_create / _free / _footprint / _edges / _max_degree and sh_rcm -- is declared in
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

SECTION = "typedef struct sh_rcm_graph sh_rcm_graph;"
WANT = {
    "sh_rcm_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_rcm_graph * *"],
    "sh_rcm_graph_free": ["sh_engine *", "sh_rcm_graph *"],
    "sh_rcm_graph_footprint": ["const sh_rcm_graph *", "uint64_t *"],
    "sh_rcm_graph_edges": ["const sh_rcm_graph *", "int64_t *"],
    "sh_rcm_graph_max_degree": ["const sh_rcm_graph *", "int64_t *"],
    "sh_rcm": ["sh_engine *", "sh_rcm_graph *", "sh_vec *", "sh_vec *", "sh_vec *", "int32_t", "int32_t", "int32_t",
               "int32_t *", "int32_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "int64_t *",
               "int32_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}
KERNELS = ("rcm_init", "rcm_begin", "rcm_sweep", "rcm_claim", "rcm_count", "rcm_place", "rcm_close", "rcm_finish", "rcm_total")
FOOTPRINT = "4 * (rows + 1) + 28 * rows + 8 * edges + 50176"


def test_rcm_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "SIMPLE UNDIRECTED", "the smaller pair (deg, index)", "George and Liu",
                 "With sweeps == 0 that is all", "if x == r stop", "if e' > e take r = x", "position k becomes rows - 1 - k",
                 "A[perm][:, perm] is the reordered matrix", "the inverse of perm", "takes no step", "exact, 64-bit",
                 "a search of eccentricity e takes e + 1 steps", "at most (sweeps + 2) * rows steps", "every comparison is ==",
                 "atomicMin(owner[w], i)", "The order array is its own queue", "nothing is sorted per level",
                 "generations count down", "five launches", "a ballot prefix", "in chunks of 256",
                 "crosses a launch boundary", "no compare-and-swap, no spin and no flag", "Worst cases", "NOT covered",
                 "Sloan", "nested dissection", FOOTPRINT, "sweeps outside [0, 64]", "reverse outside {0, 1}", "max_steps < 1",
                 "the scalars are checked first", "before any device work", "Freeing NULL is SH_OK", "rows == 0",
                 "the rest of perm is -1", "*bandwidth_after and *profile_after are -1",
                 "one handle serves any number of calls, one at a time"):
        assert cite in comment, cite
    assert "@" not in comment and "GO_HERE" not in comment


def footprint_of(text):
    """The formula the header states, as a function of rows and edges."""
    m = re.search(r"sh_rcm_graph_footprint: device bytes held = 4 \* \(rows \+ 1\) \+ (\d+) \* rows \+ (\d+) \* edges \+ (\d+)\.", text)
    assert m, "the header states no footprint formula for sh_rcm_graph"
    a, b, c = (int(x) for x in m.groups())
    return lambda rows, edges: 4 * (rows + 1) + a * rows + b * edges + c


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_rcm_gpu.py compares sh_rcm_graph_footprint with is the header's, and its numbers are those of
    rcm.hip.h: S, order, posl, levl, stamp, owner and cnt (4 bytes per row each), the lists (8 bytes per edge), the control
    block, one WlPart (16 bytes) and one RcmFin (32 bytes) per workgroup."""
    f = footprint_of(" ".join(section_comment(SECTION, stars=False).split()))
    import test_rcm_gpu
    for rows, edges in ((0, 0), (1, 0), (60, 59), (160_000, 319_200)):
        assert f(rows, edges) == test_rcm_gpu.header_footprint(rows, edges) == 4 * (rows + 1) + 28 * rows + 8 * edges + 50176
    code = open(os.path.join(CSRC, "rcm.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("RCM_LANE", "RCM_WAVE", "RCM_BATCH", "RCM_MAX_BLOCKS", "RCM_CTL_BYTES", "RCM_MAX_SWEEPS")}
    assert const["RCM_CTL_BYTES"] + (16 + 32) * const["RCM_MAX_BLOCKS"] == 50176
    assert const["RCM_BATCH"] == 32 and const["RCM_MAX_SWEEPS"] == 64
    import rcm_ref
    assert (const["RCM_LANE"], const["RCM_WAVE"]) == (rcm_ref.LANE, rcm_ref.WAVE) and rcm_ref.BATCHES[-1] == const["RCM_BATCH"]
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "RCM_CTL_BYTES + RCM_PART_BYTES + RCM_FIN_BYTES == 50176" in hip
    assert "int32_t it = 0, batch = 8;" in hip   # (run_batches: what rcm_ref.BATCHES starts with)
    assert "#define SH_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sparseharness_hip.h")).read()


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device, the scalars first, and no output is written."""
    lib = abi.load()
    check_create_errors("sh_rcm_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_rcm_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_rcm_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_rcm_graph_max_degree(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_rcm_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    i32 = [C.c_int32(7) for _ in range(4)]
    i64 = [C.c_int64(7) for _ in range(4)]
    outs = [C.byref(x) for x in i32 + i64]

    def call(sweeps=8, reverse=1, max_steps=100):
        return lib.sh_rcm(None, None, None, None, None, sweeps, reverse, max_steps, *outs, *(None,) * 5)

    for sweeps in (-1, 65, 1000):
        assert call(sweeps=sweeps) == abi.SH_EINVAL and "sweeps" in last_error() and "sh_rcm" in last_error()
    for reverse in (-1, 2):
        assert call(reverse=reverse) == abi.SH_EINVAL and "reverse" in last_error() and "sh_rcm" in last_error()
    for max_steps in (0, -5):
        assert call(max_steps=max_steps) == abi.SH_EINVAL and "max_steps" in last_error() and "sh_rcm" in last_error()
    assert call(sweeps=65, reverse=2, max_steps=0) == abi.SH_EINVAL and "sweeps" in last_error()   # in that order
    for sweeps, reverse, max_steps in ((0, 0, 1), (8, 1, 1 << 20), (64, 1, 7)):   # legal scalars: the NULL handles are next
        assert call(sweeps, reverse, max_steps) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "perm", "components", "sweeps_run", "steps", "complete", "bandwidth", "profile"):
            assert word in last_error()
    assert [x.value for x in i32 + i64] == [7] * 8   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("RCM_KERNELS", "seen_rcm", "match_bid", "gcol_assign", "truss_peel"):
        assert k in src
    assert "len(seen_rcm) != len(RCM_KERNELS)" in src and "offenders" in src
    assert len(re.search(r"RCM_KERNELS = \(([^)]*)\)", src).group(1).split(",")) == len(KERNELS)
    assert "rcm.hip.h" in open(os.path.join(CSRC, "Makefile")).read()
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "rcm.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_rcm: step\"", "create_graph_handle<sh_rcm_graph>(e, RCM_CREATE",
                        "RCM_CREATE = \"sh_rcm_graph_create\"", "struct sh_rcm_graph : GraphHandle<RcmCtl>"):
        assert k in hip, k
    assert hip.count("int sh_rcm_graph_free(sh_engine *e, sh_rcm_graph *g) { return free_handle(e, g); }") == 1
    assert hip.count("build_und_edges(e, scratch, ") == 1   # the edges under the entries are found by the code of sh_tri and sh_core
    code = open(os.path.join(CSRC, "rcm.hip.h")).read()
    for phrase in ("LABEL SPACE", "THE LEVEL FORM IS THE SERIAL FORM", "EVERY VERTEX GETS ONE POSITION", "NO KERNEL EVER WAITS",
                   "EVERY LOOP IS BOUNDED", "Cuthill, McKee", "George, Liu", "Worst cases"):
        assert phrase in " ".join(code.replace("//", " ").split()), phrase   # (a phrase may run over a comment's line break)
    for k in KERNELS + ("struct RcmCtl", "RcmRec rec[RCM_BATCH]", "wl_append_here"):
        assert k in code, k
    body = code.split("#pragma once")[1]
    # the parts and the closing sums go through the shared folds, and the header defines no workgroup fold of its own:
    # what is left of shuffles and per-wave words ranks entries (rcm_tile, rcm_block_scan), it folds nothing
    for k in ("wl_block_part(part, 0u, looked)", "wl_block_part(part, total, looked)", "wl_sum_parts(part, nparts)",
              "wl_block_fold<WlMax>(bw0)", "wl_block_fold<WlSum>(prof0)", "wl_block_fold<WlMax>(f.bw[k])",
              "wl_block_fold<WlSum>(f.prof[k])"):
        assert k in body, k
    assert "__shfl_xor" not in body and "_block_part(WlPart" not in body and "_sum_parts(const" not in body
    words = re.findall(r"__shared__[^;]*\[WL_BS(?: / 64)?\](?!\[)[^;]*;", body)
    assert len(words) == 2 and "s_wcnt[WL_BS / 64]" in words[0] and "s_w[WL_BS / 64]" in words[1], words
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "while (true)" not in body and "for (;;)" not in body        # no spin
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/rcm_order.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_rcm_order" in open(os.path.join(host, "inc", "sh_host.h")).read()
    gold = open(os.path.join(host, "src", "rcm_order.cpp")).read()
    assert "owner" not in gold and "std::sort" in gold   # the definition keeps one queue; it claims nothing


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    n, o, seven = text.index("## 6n."), text.index("## 6o."), text.index("\n## 7")
    assert n < o < seven
    section = text[o:text.index("\n## ", o + 1)]
    assert section.startswith("## 6o. Reverse Cuthill-McKee (`sh_rcm_graph_create`, `sh_rcm`)")
    for part in ("Layout", "Schedule", "Why the level form is the serial form", "Worst cases", "Measurements", "Calling rule",
                 "Not covered"):
        assert "**" + part in section, part
    assert "GO_HERE" not in section and "TODO" not in section and "@" not in section
    for word in ("sh_rcm_graph_create", "rcm_bench.py", "atomicMin(owner[w], i)", "synth:grid-2048", "synth:rmat-18",
                 "synth:scircuit", "hostlib.rcm_order", "sh_spmv", FOOTPRINT):
        assert word in section, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.rcm_graph(" in readme and "eng.rcm_order(" in readme and "6o" in readme
    assert "rcm_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "rcm_bench.py"))


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.rcm import RcmGraph
    assert callable(Engine.rcm_graph) and callable(Engine.rcm_order) and callable(hostlib.rcm_order)
    assert issubclass(RcmGraph, engine._Graph) and callable(RcmGraph.free) and RcmGraph._c == "sh_rcm_graph"
    assert not hasattr(engine, "RcmGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_rcm_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in RcmGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64, "max_degree": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_rcm_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_rcm_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.rcm_order)
    assert list(sig.parameters) == ["self", "G", "perm", "pos", "level", "sweeps", "reverse", "max_steps"]
    defaults = {name: p.default for name, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"pos": None, "level": None, "sweeps": 8, "reverse": 1, "max_steps": None}
    assert list(inspect.signature(hostlib.rcm_order).parameters) == ["row_ptr", "col_idx", "val", "sweeps", "reverse", "records"]
    # a star with its hub at index 0 and three leaves: the walk starts at leaf 1 (degree 1), whose search ends in leaf 2;
    # the search from 2 is no longer, so 1 stays the root: 1, 0, 2, 3, reversed
    rp, ci = np.array([0, 3, 3, 3, 3], np.int32), np.array([1, 2, 3], np.int32)
    perm, pos, level, bw0, bw1, p0, p1, comps, searches = hostlib.rcm_order(rp, ci, np.ones(3, np.float32))
    assert perm.tolist() == [3, 2, 0, 1] and pos.tolist() == [2, 3, 1, 0] and level.tolist() == [1, 0, 2, 2]
    # (profile: the hub at position 2 reaches back to 0, leaf 1 at position 3 to the hub at 2: 2 + 1)
    assert (bw0, bw1, p0, p1, comps, searches) == (3, 2, 6, 3, 1, 2)
