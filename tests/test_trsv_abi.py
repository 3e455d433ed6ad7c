"""sh_trsv -- sh_trsv_graph_create / _free / _footprint / _entries / _levels / _max_list / _max_width / _zero_diag /
_first_zero / _level and sh_trsv -- is declared in include/sparseharness_hip.h with the agreed parameter lists, exported by
the library and bound in abi.SIGNATURES with the declared argument types; argument errors come back before any device is
touched; the kernels of trsv.hip.h are the ones the resource check counts.  No compute is called here (no GPU needed)."""
import ctypes as C
import glob
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import trsv_ref as T
from abi_checks import CSRC, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

SECTION = "typedef struct sh_trsv_graph sh_trsv_graph;"
GET = ["const sh_trsv_graph *", "int64_t *"]
WANT = {
    "sh_trsv_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *", "int32_t",
                             "int32_t", "sh_trsv_graph * *"],
    "sh_trsv_graph_free": ["sh_engine *", "sh_trsv_graph *"],
    "sh_trsv_graph_footprint": ["const sh_trsv_graph *", "uint64_t *"],
    "sh_trsv_graph_entries": GET, "sh_trsv_graph_levels": GET, "sh_trsv_graph_max_list": GET, "sh_trsv_graph_max_width": GET,
    "sh_trsv_graph_zero_diag": GET, "sh_trsv_graph_first_zero": GET,
    "sh_trsv_graph_level": ["sh_engine *", "sh_trsv_graph *", "sh_vec *"],
    "sh_trsv": ["sh_engine *", "sh_trsv_graph *", "const sh_vec *", "sh_vec *", "int32_t", "int32_t", "int64_t *", "int64_t *",
                "int64_t *", "uint64_t *"],
}
KERNELS = ("trsv_flag", "trsv_keys", "trsv_diag", "trsv_flip", "trsv_seed", "trsv_settle", "trsv_close", "trsv_rank_keys",
           "trsv_order", "trsv_level", "trsv_run")
FOOTPRINT = "4 * (rows + 1) + 24 * rows + 8 * entries + 4 * (levels + 1) + 17408"


def test_trsv_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_definition_and_what_it_leaves_out():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    for cite in ("the reference has no counterpart", "THE DEFINITION IS PART OF THE ABI", "whatever its value", "nothing is refused",
                 "Entries of the other triangle and columns out of range are ignored", "Rows need not be sorted",
                 "ascending (column, position as given)", "parallel entries stay separate terms", "a missing diagonal is +0.0",
                 "1 + the largest level[c]", "ascending (level, index)", "(b[r] - S_r) / d[r]", "(double)val_j * x[col_j]",
                 "no fused multiply-add", "pieces of 2048 entries", "64 strided partials", "for o = 32, 16, 8, 4, 2, 1",
                 "left to right", "THE TERMS ARE SIGNED", "p_k = +0.0 + t_k", "ONE function", "every comparison is ==",
                 "a NaN standing where a NaN stands", "rounded once on the way out", "read the unrounded float64 value",
                 "b and x may be the same vector", "no compare-and-swap", "one owner per x[r]", "no float atomics",
                 "ONE workgroup", "at workgroup scope", "no agent fence, no flag, no spin", "SH_TRSV_RUN = 1024",
                 "thin == 0 gives one launch per level", "the default, 256", "x does not depend on thin", "Worst cases",
                 "a host loop wins", "NOT covered", "several right-hand sides", "the transposed solve", "factorisation",
                 "the multi-GPU driver", FOOTPRINT, "Freeing NULL is SH_OK", "rows == 0 gives a valid handle",
                 "the scalars are checked first", "before any launch"):
        assert cite in comment, cite
    assert "@" not in comment and "GO_HERE" not in comment and "TODO" not in comment


def test_footprint_formula_and_constants_match_the_source():
    comment = " ".join(section_comment(SECTION, stars=False).split())
    m = re.search(r"sh_trsv_graph_footprint: device bytes held = (\d+) \* \(rows \+ 1\) \+ (\d+) \* rows \+ (\d+) \* entries \+ "
                  r"(\d+) \* \(levels \+ 1\) \+ (\d+)\.", comment)
    assert m, "the header states no footprint formula for sh_trsv_graph"
    a, b, c, d, e = (int(x) for x in m.groups())
    for rows, entries, levels in ((0, 0, 0), (1, 0, 1), (100, 198, 7), (4_194_304, 8_384_512, 4095)):
        assert a * (rows + 1) + b * rows + c * entries + d * (levels + 1) + e == T.header_footprint(rows, entries, levels)
    code = open(os.path.join(CSRC, "trsv.hip.h")).read()
    const = {k: int(eval(re.search(r"constexpr int " + k + r" = ([^;]+);", code).group(1).replace("<<", "<<")))
             for k in T.constants()}
    assert const == T.constants()
    assert const["TRSV_CTL_BYTES"] + 16 * const["TRSV_MAX_BLOCKS"] == 17408
    assert int(re.search(r"#define SH_TRSV_RUN (\d+)", code).group(1)) == T.RUN
    from sparseharness_amd import trsv
    assert (trsv.TRSV_RUN, trsv.TRSV_THIN, trsv.TRSV_THIN_MAX) == (T.RUN, T.THIN, T.THIN_MAX)
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert "TRSV_CTL_BYTES + TRSV_PART_BYTES == 17408" in hip
    gold = open(os.path.join(ROOT, "sparseharness_amd", "host", "src", "trsv_solve.cpp")).read()
    assert "PIECE = %d;" % const["TRSV_PIECE"] in gold


def test_argument_errors_need_no_device():
    """Every argument error the scalars and the host arrays decide comes back with a message that names the argument
    before anything touches a device, the scalars first, and no output is written."""
    lib = abi.load()
    check_create_errors("sh_trsv_graph_create", extra_args=(0, 0))
    check_create_errors("sh_trsv_graph_create", extra_args=(1, 1))
    rp, ci, va = np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for uplo, unit, word in ((2, 0, "uplo"), (-1, 0, "uplo"), (0, 2, "unit"), (1, -1, "unit"), (7, 7, "uplo")):
        h = C.c_void_p(1)
        assert lib.sh_trsv_graph_create(None, 1, 1, p(rp), p(ci), p(va), uplo, unit, C.byref(h)) == abi.SH_EINVAL
        assert word in last_error() and "sh_trsv_graph_create" in last_error() and not h.value
    # the scalars come before the arrays
    assert lib.sh_trsv_graph_create(None, -1, 1, None, None, None, 3, 0, None) == abi.SH_EINVAL and "uplo" in last_error()
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_trsv_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    for name in ("entries", "levels", "max_list", "max_width", "zero_diag", "first_zero"):
        assert getattr(lib, "sh_trsv_graph_" + name)(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_trsv_graph_level(None, None, None) == abi.SH_EINVAL and "sh_trsv_graph_level" in last_error()
    assert lib.sh_trsv_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    launches, runs, in_runs, total = C.c_int64(7), C.c_int64(7), C.c_int64(7), C.c_uint64(7)

    def call(f32=0, thin=-1):
        return lib.sh_trsv(None, None, None, None, f32, thin, C.byref(launches), C.byref(runs), C.byref(in_runs), C.byref(total))

    for f32 in (-1, 2):
        assert call(f32=f32) == abi.SH_EINVAL and "f32" in last_error() and "sh_trsv" in last_error()
    assert call(thin=T.THIN_MAX + 1) == abi.SH_EINVAL and "thin" in last_error()
    assert call(f32=2, thin=T.THIN_MAX + 1) == abi.SH_EINVAL and "f32" in last_error()   # in that order
    for f32, thin in ((0, -1), (1, 0), (0, T.THIN_MAX), (1, -5)):   # legal scalars: the NULL handles are next
        assert call(f32, thin) == abi.SH_EINVAL and "NULL" in last_error()
        for word in ("engine", "graph", "b", "x"):
            assert word in last_error()
    assert (launches.value, runs.value, in_runs.value, total.value) == (7, 7, 7, 7)   # nothing was written


def test_without_a_device_the_calls_fail_as_the_engine_does():
    lib = abi.load()
    if lib.sh_device_count() > 0:
        pytest.skip("a HIP device is present")
    from sparseharness_amd.engine import Engine, EngineError
    with pytest.raises(EngineError):
        Engine(0).trsv_graph(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, np.float32))


def test_resource_check_and_kernel_file():
    src = open(os.path.join(CSRC, "check_resources.py")).read()
    for k in KERNELS + ("TRSV_KERNELS", "seen_trsv", "bc_delta", "rcm_place"):
        assert k in src
    assert "len(seen_trsv) != len(TRSV_KERNELS)" in src and "offenders" in src
    listed = tuple(x.strip().strip('"') for x in re.search(r"TRSV_KERNELS = \(([^)]*)\)", src).group(1).split(","))
    code = open(os.path.join(CSRC, "trsv.hip.h")).read()
    assert sorted(listed) == sorted(re.findall(r"^__global__ (?:__launch_bounds__\(\w+\) )?void (\w+)\(", code, re.M)) == sorted(KERNELS)
    assert "trsv.hip.h" in open(os.path.join(CSRC, "Makefile")).read()
    hip = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "trsv.hip.h"' in hip
    for k in KERNELS + ("run_batches(e, \"sh_trsv_graph_create: round\"", "create_graph_handle<sh_trsv_graph>(e, TRSV_CREATE",
                        "struct sh_trsv_graph : GraphHandle<TrsvCtl>", "device_sort_pairs_u64_u32", "static void trsv_plan("):
        assert k in hip, k
    assert hip.count("int sh_trsv_graph_free(sh_engine *e, sh_trsv_graph *g) { return free_handle(e, g); }") == 1
    flat = " ".join(code.replace("//", " ").split())
    for phrase in ("THE SUM OF A LIST", "ONE OWNER PER VALUE", "NO KERNEL EVER WAITS", "EVERY LOOP IS BOUNDED", "Worst cases",
                   "NOT __restrict__", "at workgroup scope"):
        assert phrase in flat, phrase
    body = code.split("#pragma once")[1]
    for k in ("struct TrsvCtl", "TrsvRec rec[TRSV_BATCH]", "wl_append_here", "wl_expand<TRSV_LANE, TRSV_PIECE>",
              "wl_block_part(part, looked, 0u)", "wl_sum_parts(part, nparts)", "wl_from_thread0(ctl->step == L)",
              "k < len ? 0.0 + t[k] : 0.0"):
        assert k in body, k
    assert body.count("__shfl_xor") == 1 and "trsv_butterfly" in body and "__shared__" not in body
    assert body.count("__syncthreads()") == 1   # the barrier between the levels of a run, and nothing else
    # x is written and read inside trsv_run: never restrict, never a read-only or non-temporal load
    io = body[body.index("struct TrsvIo"):body.index("};", body.index("struct TrsvIo"))]
    assert "__restrict__" not in io and "nontemporal" not in body and "__ldg" not in body
    assert "asm" not in body.replace("amdgcn", "")   # plain C++ and builtins only
    assert "compare_exchange" not in body and "atomicCAS" not in body   # no compare-and-swap, no retry
    assert "while (true)" not in body and "for (;;)" not in body        # no spin
    assert not re.search(r"atomic\w*\((?:[^;]*)(?:double|float)", body) and "atomicAdd" not in body   # no float atomics
    assert "__threadfence" not in body and '"agent"' not in body        # no agent fences
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("-ffp-contract=off") >= 4 and "fast-math" not in mk and "-Ofast" not in mk
    assert "rcp" not in body and "__fdividef" not in body and "fma" not in body.lower().replace("format", "")
    host = os.path.join(ROOT, "sparseharness_amd", "host")
    assert "src/trsv_solve.cpp" in open(os.path.join(host, "Makefile")).read()
    assert "sh_trsv_solve" in open(os.path.join(host, "inc", "sh_host.h")).read()


def test_the_resource_check_counts_the_kernels_and_finds_no_offender():
    """make asm-check with the new count (the report is reused when it is newer than every source it was made from)."""
    report = os.path.join(CSRC, "build", "sh_resource_usage.txt")
    sources = [os.path.join(CSRC, "engine.hip")] + glob.glob(os.path.join(CSRC, "*.h"))
    if os.path.exists(report) and all(os.path.getmtime(report) > os.path.getmtime(s) for s in sources):
        r = subprocess.run([sys.executable, os.path.join(CSRC, "check_resources.py"), report], capture_output=True, text=True)
    else:
        r = subprocess.run(["make", "-s", "-C", CSRC, "asm-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-600:]
    assert f"{len(KERNELS)} triangular-solve" in r.stdout and "0 offenders" in r.stdout
    text = open(report).read()
    for k in KERNELS:
        assert re.search(r"Function Name: \S*" + k, text), k


def test_design_section_and_pointers():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    p, q, seven = text.index("## 6p."), text.index("## 6q."), text.index("\n## 7")
    assert p < q < seven
    section = text[q:text.index("\n## ", q + 1)]
    assert section.startswith("## 6q. Sparse triangular solve (`sh_trsv_graph_create`, `sh_trsv`)")
    for part in ("Definition", "Layout", "Schedule", "The sum", "Why the barrier form is sound", "Worst cases", "Measurements",
                 "Not covered"):
        assert "**" + part in section, part
    assert "GO_HERE" not in section and "TODO" not in section and "@" not in section
    flat = " ".join(section.split())
    for word in ("sh_trsv_graph_create", "trsv_bench.py", "hostlib.trsv_solve", "trsv_level", "trsv_run", "TRSV_RUN", "thin",
                 "synth:grid-2048", "sh_color", FOOTPRINT):
        assert word in flat, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eng.trsv_graph(" in readme and "eng.trsv(" in readme and "6q" in readme
    assert "trsv_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "trsv_bench.py"))


def test_the_python_face_exists():
    from sparseharness_amd import engine, hostlib
    from sparseharness_amd.engine import Engine
    from sparseharness_amd.trsv import TrsvGraph
    assert callable(Engine.trsv_graph) and callable(Engine.trsv) and callable(hostlib.trsv_solve) and callable(TrsvGraph.level)
    assert issubclass(TrsvGraph, engine._Graph) and callable(TrsvGraph.free) and TrsvGraph._c == "sh_trsv_graph"
    assert not hasattr(engine, "TrsvGraph")   # (tests/test_abi.py pins the handle classes of engine.py)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert abi.SIGNATURES["sh_trsv_graph_free"] == (C.c_int, [vp, vp])
    reads = {}
    for klass in TrsvGraph.__mro__:
        for attr in vars(klass).values():
            if isinstance(attr, property) and hasattr(attr.fget, "reads"):
                reads.setdefault(*attr.fget.reads)
    reads.pop("edges")   # (_Graph's name for the entries: TrsvGraph.edges reads sh_trsv_graph_entries)
    assert TrsvGraph.edges is TrsvGraph.entries
    assert reads == {"footprint": C.c_uint64, "entries": i64, "levels": i64, "max_list": i64, "max_width": i64, "zero_diag": i64,
                     "first_zero": i64}
    for suffix, ctype in reads.items():
        assert abi.SIGNATURES[f"sh_trsv_graph_{suffix}"] == (C.c_int, [vp, C.POINTER(ctype)]), suffix
    assert abi.SIGNATURES["sh_trsv_graph_create"] == (C.c_int, [vp, i64, i64, vp, vp, vp, i32, i32, C.POINTER(vp)])
    assert abi.SIGNATURES["sh_trsv_graph_level"] == (C.c_int, [vp, vp, vp])
    sig = inspect.signature(Engine.trsv)
    assert list(sig.parameters) == ["self", "G", "b", "x", "f32", "thin"]
    assert {n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == {"f32": 0, "thin": None}
    sig = inspect.signature(Engine.trsv_graph)
    assert list(sig.parameters) == ["self", "row_ptr", "col_idx", "val", "uplo", "unit"]
    assert list(inspect.signature(hostlib.trsv_solve).parameters) == ["row_ptr", "col_idx", "val", "b", "uplo", "unit", "f32"]
    # [[2, 0], [1, 4]] x = [2, 9]
    rp, ci = np.array([0, 1, 3], np.int32), np.array([0, 0, 1], np.int32)
    x, level, fig = hostlib.trsv_solve(rp, ci, np.array([2.0, 1.0, 4.0], np.float32), [2.0, 9.0])
    assert x.tolist() == [1.0, 2.0] and level.tolist() == [0, 1]
    assert fig == dict(entries=1, levels=2, max_list=1, max_width=1, zero_diag=0, first_zero=-1)
