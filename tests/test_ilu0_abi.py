"""sh_ilu0 -- sh_ilu0_graph_create / _free / _footprint / _entries / _levels / _max_list / _max_width / _missing_diag /
_first_missing / _work / _level and sh_ilu0 -- is declared in include/sparseharness_hip.h with the agreed parameter lists,
exported by the library and bound in abi.SIGNATURES with the declared argument types; argument errors come back before
any device is touched; the kernels of ilu0.hip.h are the ones the resource check counts, and the file keeps to what its
header promises.  No compute is called here (no GPU needed)."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ilu0_ref as R
from abi_checks import CSRC, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_ilu0_graph sh_ilu0_graph;"
GET = ["const sh_ilu0_graph *", "int64_t *"]
WANT = {
    "sh_ilu0_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "sh_ilu0_graph * *"],
    "sh_ilu0_graph_free": ["sh_engine *", "sh_ilu0_graph *"],
    "sh_ilu0_graph_footprint": ["const sh_ilu0_graph *", "uint64_t *"],
    "sh_ilu0_graph_entries": GET, "sh_ilu0_graph_levels": GET, "sh_ilu0_graph_max_list": GET, "sh_ilu0_graph_max_width": GET,
    "sh_ilu0_graph_missing_diag": GET, "sh_ilu0_graph_first_missing": GET, "sh_ilu0_graph_work": GET,
    "sh_ilu0_graph_level": ["sh_engine *", "sh_ilu0_graph *", "sh_vec *"],
    "sh_ilu0": ["sh_engine *", "sh_ilu0_graph *", "sh_vec *", "sh_vec *", "int32_t", "int32_t", "int64_t *", "int64_t *",
                "int64_t *", "int64_t *", "int64_t *", "uint64_t *"],
}
KERNELS = ("ilu0_flag", "ilu0_keys", "ilu0_slots", "ilu0_diag", "ilu0_work", "ilu0_load", "ilu0_level", "ilu0_run", "ilu0_store")
FOOTPRINT = "4 * (rows + 1) + 20 * rows + 12 * nnz + 16 * entries + 4 * (levels + 1) + 20"


def test_ilu0_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_definition_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "THE DEFINITION IS PART OF THE ABI", "the distinct columns c with 0 <= c < rows",
                 "in ascending c", "Rows need not be sorted", "take no part", "nothing is refused",
                 "added left to right from +0.0", "Row-wise IKJ, all in float64", "w[k] = w[k] / u[k, k]",
                 "+0.0 if row k has no diagonal slot", "w[j] = w[j] - w[k] * u[k, j]", "no fused multiply-add",
                 "the unit diagonal of L is not stored", "in ascending k, one after the other",
                 "whatever the tier, the grid or thin", "what IEEE gives", "every comparison is ==",
                 "a NaN standing where a NaN stands", "the first entry as given of its (r, c) group",
                 "uplo = 0, unit = 1", "uplo = 1, unit = 0", "each rounded once on the way out",
                 "val and lu may be the same vector when f32 == 1", "1 + the largest level among its lower slots",
                 "a missing diagonal slot counts as +0.0", "NaN pivot does not count", "-1 if there is none",
                 "no compare-and-swap", "One owner per value", "no float atomics", "ONE workgroup", "at workgroup scope",
                 "at wavefront scope", "no agent fence, no flag, no spin", "ILU0_LANE_WORK = 256", "the sweep's choice among 16, 64, 256, 1024 and 4096",
                 "thin == 0 gives one launch per level", "the default, 256", "Worst cases", "a host loop wins", "NOT covered",
                 "IC(0), ILU(k), ILUT, pivoting and diagonal shifts", "refreshing a sh_trsv handle's values on the device",
                 "a workgroup tier for hub rows", FOOTPRINT, "Freeing NULL is SH_OK", "rows == 0 or nnz == 0 give a valid handle",
                 "one handle serves any number of sh_ilu0 calls", "the scalars are checked first", "before any launch"):
        assert cite in comment, cite
    assert "@" not in comment and "GO_HERE" not in comment and "TODO" not in comment


def test_footprint_formula_and_constants_match_the_source():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    m = re.search(r"sh_ilu0_graph_footprint: device bytes held = (\d+) \* \(rows \+ 1\) \+ (\d+) \* rows \+ (\d+) \* nnz \+ "
                  r"(\d+) \* entries \+ (\d+) \* \(levels \+ 1\) \+ (\d+)\.", comment)
    assert m, "the header states no footprint formula for sh_ilu0_graph"
    a, b, c, d, e, f = (int(x) for x in m.groups())
    for rows, nnz, entries, levels in ((0, 0, 0, 0), (1, 0, 0, 1), (100, 500, 480, 7), (4_194_304, 20_963_328, 20_963_328, 4095)):
        assert a * (rows + 1) + b * rows + c * nnz + d * entries + e * (levels + 1) + f == R.header_footprint(rows, nnz, entries, levels)
    code = open(os.path.join(CSRC, "ilu0.hip.h")).read()
    const = {k: int(eval(re.search(r"constexpr int " + k + r" = ([^;]+);", code).group(1))) for k in R.constants()}
    assert const == R.constants()
    assert int(re.search(r"#define SH_ILU0_RUN (\d+)", code).group(1)) == R.RUN
    assert int(re.search(r"#define SH_ILU0_LANE_WORK (\d+)", code).group(1)) == R.LANE_WORK
    assert "#ifndef SH_ILU0_LANE_WORK" in code and "THE DEFAULT IS THE SWEEP'S" in code   # a -D override, and where the default comes from
    from sparseharness_amd import ilu0, trsv
    assert (ilu0.ILU0_RUN, ilu0.ILU0_THIN, ilu0.ILU0_THIN_MAX, ilu0.ILU0_LANE_WORK) == (R.RUN, R.THIN, R.THIN_MAX, R.LANE_WORK)
    assert (ilu0.ILU0_THIN, ilu0.ILU0_THIN_MAX) == (trsv.TRSV_THIN, trsv.TRSV_THIN_MAX)   # thin has sh_trsv's meaning and range
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "static_assert(ILU0_FIG_BYTES == 16" in hip and FOOTPRINT in hip


def test_argument_errors_need_no_device():
    """Every argument error the scalars and the host arrays decide comes back with a message that names the argument
    before anything touches a device, the scalars first, and no output is written."""
    lib = abi.load()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def create(rows, nnz, rp, ci, out=True):
        h = C.c_void_p(1)   # (stale: the call has to clear it)
        rc = lib.sh_ilu0_graph_create(None, rows, nnz, p(rp), p(ci), C.byref(h) if out else None)
        assert (not h.value or not out) and "sh_ilu0_graph_create" in last_error()
        return rc

    rp, ci = np.array([0, 1, 3], np.int32), np.array([0, 1, 0], np.int32)
    assert create(-1, 3, rp, ci) == abi.SH_EINVAL and "rows" in last_error()
    assert create(2, -1, rp, ci) == abi.SH_EINVAL and "nnz" in last_error()
    assert create(2, 3, None, ci) == abi.SH_EINVAL and "NULL" in last_error()
    assert create(2, 3, rp, None) == abi.SH_EINVAL and "NULL" in last_error()
    assert create(2, 3, rp, ci, out=False) == abi.SH_EINVAL and "NULL" in last_error()
    assert create(2, 3, np.array([1, 1, 3], np.int32), ci) == abi.SH_ESHAPE and "row_ptr[0]" in last_error()
    assert create(2, 2, rp, ci) == abi.SH_ESHAPE and "row_ptr[rows]" in last_error()
    assert create(2, 3, np.array([0, 4, 3], np.int32), ci) == abi.SH_ESHAPE and "decreases" in last_error()
    assert create(2, 3, rp, ci) == abi.SH_EINVAL and "engine" in last_error()   # well-formed: the NULL engine is next
    assert create(2, 0, np.zeros(3, np.int32), None) == abi.SH_EINVAL and "engine" in last_error()   # no entries: no columns needed
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_ilu0_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    for name in ("entries", "levels", "max_list", "max_width", "missing_diag", "first_missing", "work"):
        assert getattr(lib, "sh_ilu0_graph_" + name)(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_ilu0_graph_level(None, None, None) == abi.SH_EINVAL and "sh_ilu0_graph_level" in last_error()
    assert lib.sh_ilu0_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    outs = [C.c_int64(7) for _ in range(5)] + [C.c_uint64(7)]

    def call(f32=1, thin=-1):
        return lib.sh_ilu0(None, None, None, None, f32, thin, *(C.byref(o) for o in outs))

    for f32 in (-1, 2):
        assert call(f32=f32) == abi.SH_EINVAL and "f32" in last_error() and "sh_ilu0" in last_error()
    assert call(thin=R.THIN_MAX + 1) == abi.SH_EINVAL and "thin" in last_error()
    assert call(f32=2, thin=R.THIN_MAX + 1) == abi.SH_EINVAL and "f32" in last_error()   # in that order
    for f32, thin in ((0, -1), (1, 0), (0, R.THIN_MAX), (1, -5)):   # legal scalars: the NULL handles are next
        assert call(f32, thin) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "val", "lu"):
            assert word in last_error()
    assert [o.value for o in outs] == [7] * 6   # nothing was written


def test_without_a_device_the_calls_fail_as_the_engine_does():
    lib = abi.load()
    if lib.sh_device_count() > 0:
        pytest.skip("a HIP device is present")
    from sparseharness_amd.engine import Engine, EngineError
    with pytest.raises(EngineError):
        Engine(0).ilu0_graph(np.array([0, 1], np.int32), np.array([0], np.int32))


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("ILU0_KERNELS", "seen_ilu0", "trsv_run", "bc_delta"):
        assert k in src
    assert "len(seen_ilu0) != len(ILU0_KERNELS)" in src and "offenders" in src
    assert src.index("incomplete-LU,") < src.index("triangular-solve and")   # the new clause stands before the old ones' end
    listed = tuple(x.strip().strip('"') for x in re.search(r"ILU0_KERNELS = \(([^)]*)\)", src).group(1).split(","))
    trsv = tuple(x.strip().strip('"') for x in re.search(r"TRSV_KERNELS = \(([^)]*)\)", src, re.S).group(1).split(","))
    assert not any(t in k for k in listed for t in trsv)   # no ilu0_ kernel is counted as a trsv_ kernel
    code = open(os.path.join(CSRC, "ilu0.hip.h")).read()
    assert sorted(listed) == sorted(re.findall(r"^__global__ (?:__launch_bounds__\(\w+\) )?void (\w+)\(", code, re.M)) == sorted(KERNELS)
    assert "ilu0.hip.h" in open(os.path.join(CSRC, "Makefile")).read()
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "ilu0.hip.h"' in hip
    for k in KERNELS + ("create_graph_handle<sh_ilu0_graph>(e, ILU0_CREATE", "struct sh_ilu0_graph : GraphBase", "build_trsv(e, &t,",
                        "device_sort_pairs_u64_u32", "trsv_plan(g->lstart, thin, ILU0_RUN, plan)", "wl_run_heads"):
        assert k in hip, k
    assert hip.count("int sh_ilu0_graph_free(sh_engine *e, sh_ilu0_graph *g) { return free_handle(e, g); }") == 1
    flat = " ".join(code.replace("//", " ").split())
    for phrase in ("THE SLOTS", "THE LEVELS", "THE ELIMINATION OF A ROW", "ONE OWNER PER VALUE", "WHY THE IN-LAUNCH FORMS ARE SOUND",
                   "NO KERNEL EVER WAITS", "EVERY LOOP IS BOUNDED", "Worst cases", "NOT __restrict__", "at workgroup scope",
                   "at wavefront scope"):
        assert phrase in flat, phrase
    body = code.split("#pragma once")[1]
    assert '#include "trsv.hip.h"' not in body and "trsv_" not in body   # its own file: nothing of trsv.hip.h is touched
    # w is written and re-read inside a launch: never restrict, never a read-only or non-temporal load
    lists = body[body.index("struct Ilu0Lists"):body.index("};", body.index("struct Ilu0Lists"))]
    assert "double *w;" in lists and "__restrict__" not in lists and "nontemporal" not in body and "__ldg" not in body
    rows = body[body.index("void ilu0_update("):body.index("__global__ __launch_bounds__(WL_BS) void ilu0_store(")]
    assert "__restrict__ lstart" in rows and rows.count("__restrict__") == 1   # (lstart alone: the host wrote it)
    assert rows.count("__syncthreads()") == 1 and body.count("__syncthreads()") == 1   # the barrier between the levels of a run
    assert rows.count("wl_wave_sync()") == 2 and "__shared__" not in body
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "while (true)" not in body and "for (;;)" not in body and "while (1)" not in body   # no spin
    assert not re.search(r"atomic\w*\((?:[^;]*)(?:double|float)", body) and "atomicAdd" not in body   # no float atomics
    assert "__threadfence" not in body and '"agent"' not in body and '"workgroup"' not in body     # no agent fences
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("-ffp-contract=off") >= 4 and "fast-math" not in mk and "-Ofast" not in mk
    assert "-DSH_ILU0_LANE_WORK=$(LANE_WORK)" in mk
    assert "rcp" not in body and "__fdividef" not in body and "fma" not in body.lower().replace("format", "")
    assert "const double p = wk * T.w[t];" in body and "T.w[lo] = T.w[lo] - p;" in body   # two roundings, written out
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/ilu0_factor.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_ilu0_factor" in open(os.path.join(host, "inc", "sh_host.h")).read()


def test_the_resource_check_counts_the_kernels_and_finds_no_offender():
    """make asm-check with the new count (the report is reused when it is newer than every source it was made from)."""
    report = os.path.join(CSRC, "build", "sh_resource_usage.txt")
    sources = [os.path.join(CSRC, "engine.hip")] + glob.glob(os.path.join(CSRC, "*.h"))
    if os.path.exists(report) and all(os.path.getmtime(report) > os.path.getmtime(s) for s in sources):
        r = subprocess.run([sys.executable, os.path.join(CSRC, "check_resources.py"), report], capture_output=True, text=True)
    else:
        r = subprocess.run(["make", "-s", "-C", CSRC, "asm-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-600:]
    assert f"{len(KERNELS)} incomplete-LU" in r.stdout and "0 offenders" in r.stdout
    text = open(report).read()
    for k in KERNELS:
        assert re.search(r"Function Name: \S*" + k, text), k


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    q, r, seven = text.index("## 6q."), text.index("## 6r."), text.index("\n## 7")
    assert q < r < seven
    section = text[r:text.index("\n## ", r + 1)]
    assert section.startswith("## 6r. Incomplete LU factorisation (`sh_ilu0_graph_create`, `sh_ilu0`)")
    for part in ("Definition", "Layout", "Schedule", "Why the in-launch forms are sound", "Worst cases", "Measurements", "Not covered"):
        assert "**" + part in section, part
    assert "GO_HERE" not in section and "TODO" not in section and "@" not in section
    flat = " ".join(section.split())
    for word in ("sh_ilu0_graph_create", "ilu0_bench.py", "hostlib.ilu0_factor", "ilu0_level", "ilu0_run", "ilu0_load", "ilu0_store",
                 "ILU0_RUN", "ILU0_LANE_WORK", "thin", "synth:grid-2048", "sh_color", "synth:scircuit", "wl_wave_sync", FOOTPRINT,
                 "2.2564e-16", "1.8052e-15", "IC(0)", "ILUT", "workgroup tier"):
        assert word in flat, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.ilu0_graph(" in readme and "eng.ilu0(" in readme and "6r" in readme
    example = readme[readme.index("eng.ilu0_graph("):]
    assert example.count("eng.trsv_graph(") >= 2   # the example ends in the two handles on the downloaded lu
    assert "ilu0_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "ilu0_bench.py"))


def test_the_python_face_exists():
    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.ilu0 import Ilu0Graph
    assert callable(Engine.ilu0_graph) and callable(Engine.ilu0) and callable(hostlib.ilu0_factor) and callable(Ilu0Graph.level)
    assert issubclass(Ilu0Graph, engine._Graph) and callable(Ilu0Graph.free) and Ilu0Graph._c == "sh_ilu0_graph"
    assert not hasattr(engine, "Ilu0Graph")   # (tests/test_abi.py pins the handle classes of engine.py)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert abi.SIGNATURES["sh_ilu0_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in Ilu0Graph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    reads.pop("edges")   # (_Graph's name for the entries: Ilu0Graph.edges reads sh_ilu0_graph_entries)
    assert Ilu0Graph.edges is Ilu0Graph.entries
    assert reads == {"footprint": C.c_uint64, "entries": i64, "levels": i64, "max_list": i64, "max_width": i64, "missing_diag": i64,
                     "first_missing": i64, "work": i64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_ilu0_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_ilu0_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, C.POINTER(vp)])
    assert abi.SIGNATURES["sh_ilu0_graph_level"] == (C.c_int, [vp, vp, vp])
    sig = inspect.signature(Engine.ilu0)
    assert list(sig.parameters) == ["self", "G", "val", "lu", "f32", "thin"]
    assert {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == {"f32": 1, "thin": None}
    assert list(inspect.signature(Engine.ilu0_graph).parameters) == ["self", "row_ptr", "col_idx"]
    sig = inspect.signature(hostlib.ilu0_factor)
    assert list(sig.parameters) == ["row_ptr", "col_idx", "val", "f32"] and sig.parameters["f32"].default == 1
    # [[2, 1], [4, 5]] = [[1, 0], [2, 1]] [[2, 1], [0, 3]]
    rp, ci = np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32)
    lu, level, fig = hostlib.ilu0_factor(rp, ci, np.array([2.0, 1.0, 4.0, 5.0], np.float32))
    assert lu.dtype == np.float32 and lu.tolist() == [2.0, 1.0, 2.0, 3.0] and level.tolist() == [0, 1]
    assert fig == dict(entries=4, levels=2, max_list=2, max_width=1, missing_diag=0, first_missing=-1, work=1, zero_pivots=0,
                       first_zero=-1)
