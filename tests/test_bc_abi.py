"""sh_bc -- sh_bc_graph_create / _free / _footprint / _edges / _max_list and sh_bc -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched; the kernels of bc.hip.h are the ones
the resource check counts.  No compute is called here (no GPU needed)."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import numpy as np

from abi_checks import CSRC, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_bc_graph sh_bc_graph;"
WANT = {
    "sh_bc_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                           "sh_bc_graph * *"],
    "sh_bc_graph_free": ["sh_engine *", "sh_bc_graph *"],
    "sh_bc_graph_footprint": ["const sh_bc_graph *", "uint64_t *"],
    "sh_bc_graph_edges": ["const sh_bc_graph *", "int64_t *"],
    "sh_bc_graph_max_list": ["const sh_bc_graph *", "int64_t *"],
    "sh_bc": ["sh_engine *", "sh_bc_graph *", "const int32_t *", "int32_t", "sh_vec *", "int32_t", "sh_vec *", "sh_vec *",
              "int64_t *", "int32_t *", "int64_t *", "double *", "int64_t *", "uint64_t *", "uint64_t *"],
}
KERNELS = ("bc_in_keys", "bc_out_keys", "bc_init", "bc_expand", "bc_count", "bc_close", "bc_delta")
FOOTPRINT = "12 * (rows + 1) + 24 * rows + 8 * edges + 16 * (edges / 1024 + 1) + 17408"


def test_bc_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "Brandes", "SIMPLE DIRECTED", "parallel entries are one edge",
                 "self-loops are none", "sigma_s(s) = 1", "(sigma(v) / sigma(w)) * (1 + delta(w))", "in the order given",
                 "Endpoints are not counted and nothing is normalised", "halving is the caller's line",
                 "A source may occur twice and then counts twice", "exact while it stays below 2^53", "+inf",
                 "Nothing is refused", "THE ORDER OF EVERY ADDITION IS PART OF THE RESULT", "SUM(list)",
                 "pieces of 2048 entries", "64 strided partials", "for o = 32, 16, 8, 4, 2, 1", "left to right",
                 "((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7))", "no fused multiply-add", "every comparison is ==",
                 "one owner per value", "There are no float atomics", "the queue order, the grid, the batch size or the run",
                 "atomicMin on the unsigned level word", "no compare-and-swap", "its own queue", "depth - 1 ... 1",
                 "takes d + 1 steps", "Worst cases", "a path pays three launches forward and one backward",
                 "pulled by one wave alone", "C(n, n / 2)", "unmeasured", "NOT covered", "several sources per matrix read",
                 "weighted shortest paths", "edge betweenness", "normalisation", "the multi-GPU driver", FOOTPRINT,
                 "accumulate outside {0, 1}", "n_sources < 0", "the scalars are checked first", "a source outside [0, rows)",
                 "not aligned to 8 bytes", "overlapping one another", "before any device work", "Freeing NULL is SH_OK",
                 "rows == 0", "n_sources == 0 is legal", "2 * rows elements are written, no more",
                 "get the bits of one call", "One handle serves any number of calls, one at a time"):
        assert cite in comment, cite
    assert "@" not in comment and "GO_HERE" not in comment


def footprint_of(text):
    """The formula the header states, as a function of rows and edges."""
    m = re.search(r"sh_bc_graph_footprint: device bytes held = (\d+) \* \(rows \+ 1\) \+ (\d+) \* rows \+ (\d+) \* edges \+ "
                  r"(\d+) \* \(edges / (\d+) \+ 1\) \+ (\d+)\.", text)
    assert m, "the header states no footprint formula for sh_bc_graph"
    a, b, c, d, e, f = (int(x) for x in m.groups())
    return lambda rows, edges: a * (rows + 1) + b * rows + c * edges + d * (edges // e + 1) + f


def test_footprint_formula_is_stated_in_the_header_and_matches_the_constants():
    """The formula tests/test_bc_gpu.py (through tests/bc_ref.py) compares sh_bc_graph_footprint with is the header's, and its numbers are those of
    bc.hip.h: in_ptr, out_ptr and the level starts (4 bytes per row + 1 each), level and order (4 per row), sigma and delta
    (8 per row), the two lists (4 bytes per edge each), two piece lists, the control block and one WlPart per workgroup."""
    f = footprint_of(" ".join(section_comment(SECTION, stars=False).split()))
    import bc_ref
    for rows, edges in ((0, 0), (1, 0), (100, 198), (262_144, 3_805_085)):
        assert f(rows, edges) == bc_ref.header_footprint(rows, edges)
    code = open(os.path.join(CSRC, "bc.hip.h")).read()
    const = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", code).group(1))
             for k in ("BC_LANE", "BC_PIECE", "BC_BATCH", "BC_MAX_BLOCKS", "BC_CTL_BYTES")}
    assert const["BC_CTL_BYTES"] + 16 * const["BC_MAX_BLOCKS"] == 17408 and const["BC_PIECE"] // 2 == 1024
    assert const["BC_BATCH"] == 32
    assert (const["BC_LANE"], const["BC_PIECE"]) == (bc_ref.LANE, bc_ref.PIECE)
    assert all(bc_ref.constants()[k] == v for k, v in const.items())
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "BC_CTL_BYTES + BC_PART_BYTES == 17408" in hip
    assert "#define SH_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sparseharness_hip.h")).read()
    gold = open(os.path.join(ROOT, "sparseharness_amd", "host", "src", "bc_scores.cpp")).read()
    assert "PIECE = %d;" % const["BC_PIECE"] in gold


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device, the scalars first, and no output is written."""
    lib = abi.load()
    check_create_errors("sh_bc_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_bc_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_bc_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_bc_graph_max_list(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_bc_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    steps, total = C.c_int64(7), C.c_uint64(7)
    src = np.zeros(2, np.int32)

    def call(n_sources=2, accumulate=0):
        return lib.sh_bc(None, None, src.ctypes.data_as(C.c_void_p), n_sources, None, accumulate, None, None, C.byref(steps),
                         None, None, None, None, None, C.byref(total))

    for accumulate in (-1, 2, 7):
        assert call(accumulate=accumulate) == abi.SH_EINVAL and "accumulate" in last_error() and "sh_bc" in last_error()
    for n_sources in (-1, -100):
        assert call(n_sources=n_sources) == abi.SH_EINVAL and "n_sources" in last_error() and "sh_bc" in last_error()
    assert call(n_sources=-1, accumulate=2) == abi.SH_EINVAL and "accumulate" in last_error()   # in that order
    for n_sources, accumulate in ((0, 0), (2, 1)):   # legal scalars: the NULL handles are next
        assert call(n_sources, accumulate) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "bc", "sources"):
            assert word in last_error()
    assert (steps.value, total.value) == (7, 7)   # nothing was written


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("BC_KERNELS", "seen_bc", "rcm_place", "match_bid", "gcol_assign"):
        assert k in src
    assert "len(seen_bc) != len(BC_KERNELS)" in src and "offenders" in src
    listed = tuple(x.strip().strip('"') for x in re.search(r"BC_KERNELS = \(([^)]*)\)", src).group(1).split(","))
    code = open(os.path.join(CSRC, "bc.hip.h")).read()
    assert sorted(listed) == sorted(re.findall(r"^__global__ (?:__launch_bounds__\(\w+\) )?void (\w+)\(", code, re.M)) == sorted(KERNELS)
    assert "bc.hip.h" in open(os.path.join(CSRC, "Makefile")).read()
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "bc.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_bc: step\"", "create_graph_handle<sh_bc_graph>(e, BC_CREATE",
                        "BC_CREATE = \"sh_bc_graph_create\"", "struct sh_bc_graph : GraphHandle<BcCtl>"):
        assert k in hip, k
    assert hip.count("int sh_bc_graph_free(sh_engine *e, sh_bc_graph *g) { return free_handle(e, g); }") == 1
    for phrase in ("THE SUM OF A LIST", "ONE OWNER PER VALUE", "NO KERNEL EVER WAITS", "EVERY LOOP IS BOUNDED", "Brandes",
                   "Worst cases"):
        assert phrase in " ".join(code.replace("//", " ").split()), phrase
    for k in KERNELS + ("struct BcCtl", "BcRec rec[BC_BATCH]", "wl_append_here", "wl_expand<BC_LANE, BC_PIECE>"):
        assert k in code, k
    body = code.split("#pragma once")[1]
    # integer sums of parts go through the layer; the one float64 fold is the header's own, in one place
    for k in ("wl_block_part(part, looked, 0u)", "wl_sum_parts(part, nparts)", "wl_from_thread0(ctl->step == L)"):
        assert k in body, k
    assert body.count("__shfl_xor") == 1 and "bc_butterfly" in body and "__shared__" not in body
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "while (true)" not in body and "for (;;)" not in body        # no spin
    assert not re.search(r"atomic\w*\((?:[^;]*)(?:double|float)", body) and "atomicAdd" not in body   # no float atomics
    # the arithmetic the == rests on: no contraction, no fast-math, no reciprocal
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("-ffp-contract=off") >= 4 and "fast-math" not in mk and "-Ofast" not in mk
    assert "rcp" not in body and "__fdividef" not in body and "fma" not in body.lower().replace("format", "")
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/bc_scores.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "-ffp-contract=off" in open(os.path.join(host, "Makefile")).read()
    assert "sh_bc_scores" in open(os.path.join(host, "inc", "sh_host.h")).read()


def test_the_resource_check_counts_the_kernels_and_finds_no_offender():
    """make asm-check with the new count (the report is reused when it is newer than every source it was made from)."""
    report = os.path.join(CSRC, "build", "sh_resource_usage.txt")
    sources = [os.path.join(CSRC, "engine.hip")] + glob.glob(os.path.join(CSRC, "*.h"))
    if os.path.exists(report) and all(os.path.getmtime(report) > os.path.getmtime(s) for s in sources):
        r = subprocess.run([sys.executable, os.path.join(CSRC, "check_resources.py"), report], capture_output=True, text=True)
    else:
        r = subprocess.run(["make", "-s", "-C", CSRC, "asm-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-600:]
    assert f"{len(KERNELS)} betweenness kernels checked, 0 offenders" in r.stdout
    text = open(report).read()
    for k in KERNELS:
        assert re.search(r"Function Name: \S*" + k, text), k


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    o, p, seven = text.index("## 6o."), text.index("## 6p."), text.index("\n## 7")
    assert o < p < seven
    section = text[p:text.index("\n## ", p + 1)]
    assert section.startswith("## 6p. Betweenness centrality (`sh_bc_graph_create`, `sh_bc`)")
    for part in ("Layout", "Schedule", "The summation order", "Why it is one function for all tiers", "Worst cases",
                 "Measurements", "Not covered"):
        assert "**" + part in section, part
    assert "GO_HERE" not in section and "TODO" not in section and "@" not in section
    flat = " ".join(section.split())   # (a phrase may run over a line break)
    for word in ("sh_bc_graph_create", "bc_bench.py", "atomicMin", "synth:grid-512", "synth:rmat-18", "synth:scircuit",
                 "hostlib.bc_scores", "sh_bfs_levels", "test_small_graphs", "not under them yet", FOOTPRINT):
        assert word in flat, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.bc_graph(" in readme and "eng.betweenness(" in readme and "6p" in readme
    assert "bc_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bc_bench.py"))


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.bc import BcGraph
    from sparseharness_amd.engine import Engine
    assert callable(Engine.bc_graph) and callable(Engine.betweenness) and callable(hostlib.bc_scores)
    assert issubclass(BcGraph, engine._Graph) and callable(BcGraph.free) and BcGraph._c == "sh_bc_graph"
    assert not hasattr(engine, "BcGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    vp, i64 = C.c_void_p, C.c_int64
    assert abi.SIGNATURES["sh_bc_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in BcGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    assert reads == {"footprint": C.c_uint64, "edges": C.c_int64, "max_list": C.c_int64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_bc_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_bc_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, C.POINTER(vp)])
    sig = inspect.signature(Engine.betweenness)
    assert list(sig.parameters) == ["self", "G", "sources", "bc", "accumulate", "sigma", "level"]
    defaults = {name: p.default for name, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == {"accumulate": 0, "sigma": None, "level": None}
    assert list(inspect.signature(hostlib.bc_scores).parameters) == ["row_ptr", "col_idx", "val", "sources", "bc"]
    # a path 0 - 1 - 2, symmetric: from every source, the middle lies on the two paths between the ends
    rp, ci = np.array([0, 1, 3, 4], np.int32), np.array([1, 0, 2, 1], np.int32)
    bc, sigma, level, depth, reached, smax, edges = hostlib.bc_scores(rp, ci, np.ones(4, np.float32), [0, 1, 2])
    assert bc.tolist() == [0.0, 2.0, 0.0] and sigma.tolist() == [1.0, 1.0, 1.0] and level.tolist() == [2, 1, 0]
    assert (depth.tolist(), reached.tolist(), smax.tolist(), edges.tolist()) == ([2, 1, 2], [3, 3, 3], [1.0] * 3, [4, 4, 4])
