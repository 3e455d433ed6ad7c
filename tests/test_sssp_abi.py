"""The bucketed SSSP -- sh_sssp_graph_create / _free / _footprint / _edges / _delta and sh_sssp -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import HEADER, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_sssp_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                             "sh_sssp_graph * *"],
    "sh_sssp_graph_free": ["sh_engine *", "sh_sssp_graph *"],
    "sh_sssp_graph_footprint": ["const sh_sssp_graph *", "uint64_t *"],
    "sh_sssp_graph_edges": ["const sh_sssp_graph *", "int64_t *"],
    "sh_sssp_graph_delta": ["const sh_sssp_graph *", "double *"],
    "sh_sssp": ["sh_engine *", "sh_sssp_graph *", "const sh_vec *", "sh_vec *", "sh_vec *", "double", "int32_t",
                "int32_t *", "int32_t *", "int64_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "uint64_t *",
                "uint64_t *"],
}


def test_sssp_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_cites_what_it_extends_and_what_it_leaves_out():
    comment = section_comment("typedef struct sh_sssp_graph sh_sssp_graph;")
    for cite in ("app/sssp.cpp:97-176", "inc/harness.h:149-195", "no counterpart", "NOT covered", "other semirings",
                 "sh_iterate_multi", "row pieces", "multi-GPU", "C++ harness apps", "Measured on an MI355X", "Rule:",
                 "sh_iterate(SH_MIN_PLUS_F32, alpha = 0, beta = 0, y0 = x0)", "A stored zero IS an edge", "FOREST",
                 "does not depend on delta", "mean out-degree", "max_rounds", "No kernel ever waits"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_sssp_gpu.py compares sh_sssp_graph_footprint with is the header's."""
    text = " ".join(open(HEADER).read().split())
    assert "8 * (rows + 1) + 16 * edges + 20 * rows + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 22528" in text


def sssp(max_rounds, delta=-1.0):
    r, b, n, c, x = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64()
    return abi.load().sh_sssp(None, None, None, None, None, delta, max_rounds, C.byref(r), C.byref(b), C.byref(n), C.byref(c),
                              C.byref(x), None, None, None, None)


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_sssp_graph_create")
    b, k, d = C.c_uint64(), C.c_int64(), C.c_double()
    assert lib.sh_sssp_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_sssp_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_sssp_graph_delta(None, C.byref(d)) == abi.SH_EINVAL
    assert lib.sh_sssp_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    for cap in (0, -3):
        assert sssp(cap) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert sssp(10, delta=float("nan")) == abi.SH_EINVAL and "delta" in last_error() and "NaN" in last_error()
    assert sssp(10) == abi.SH_EINVAL and "NULL" in last_error() and "x0" in last_error()
    assert sssp(10, delta=float("inf")) == abi.SH_EINVAL and "NULL" in last_error()   # (an infinite width is legal)
    assert sssp(10, delta=0.0) == abi.SH_EINVAL and "NULL" in last_error()            # (and so is "the default")


def test_resource_check_covers_the_sssp_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in ("sssp_init", "sssp_relax", "sssp_split", "sssp_decide", "sssp_preds", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "sssp.hip.h" in mk
    hip = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "engine.hip")).read()
    assert '#include "sssp.hip.h"' in hip


def test_the_python_face_exists():
    from sparseharness_amd.engine import Engine, SsspGraph
    assert callable(Engine.sssp_graph) and callable(Engine.sssp) and hasattr(SsspGraph, "delta")
