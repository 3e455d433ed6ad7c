"""sh_scc -- sh_scc_graph_create / _free / _footprint / _edges and sh_scc -- is declared in include/sparseharness_hip.h
with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the declared argument types;
argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import HEADER, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_scc_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_scc_graph * *"],
    "sh_scc_graph_free": ["sh_engine *", "sh_scc_graph *"],
    "sh_scc_graph_footprint": ["const sh_scc_graph *", "uint64_t *"],
    "sh_scc_graph_edges": ["const sh_scc_graph *", "int64_t *"],
    "sh_scc": ["sh_engine *", "sh_scc_graph *", "sh_vec *", "int32_t", "int32_t", "int32_t", "int64_t *", "int64_t *",
               "int64_t *", "int32_t *", "int32_t *", "int32_t *", "int32_t *", "int64_t *", "int32_t *", "int64_t *",
               "uint64_t *", "uint64_t *"],
}


def test_scc_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_cites_what_it_extends_and_what_it_leaves_out():
    comment = section_comment("typedef struct sh_scc_graph sh_scc_graph;")
    for cite in ("app/scc.cpp:96-176", "inc/harness.h:149-195", "no counterpart", "NOT covered", "largest", "does not depend on",
                 "No kernel ever waits", "Measured on an MI355X", "Rule:", "other semirings", "row pieces", "multi-GPU",
                 "C++ harness apps", "weakly connected", "serial tail", "max_steps"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_scc_gpu.py compares sh_scc_graph_footprint with is the header's."""
    text = " ".join(open(HEADER).read().split())
    assert "8 * (rows + 1) + 8 * edges + 20 * rows + 32 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 34816" in text


def scc(max_steps):
    k, s, t, r, n, c = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
    return abi.load().sh_scc(None, None, None, 1, 1, max_steps, C.byref(k), C.byref(s), C.byref(t), C.byref(r), C.byref(n),
                             C.byref(c), None, None, None, None, None, None)


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_scc_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_scc_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_scc_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_scc_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    for cap in (0, -3):
        assert scc(cap) == abi.SH_EINVAL and "max_steps" in last_error()
    assert scc(10) == abi.SH_EINVAL and "NULL" in last_error() and "comp" in last_error()


def test_resource_check_covers_the_scc_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in ("scc_init", "scc_trim", "scc_pick", "scc_seed", "scc_propagate", "scc_claim", "scc_label", "scc_decide",
              "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "scc.hip.h" in mk
    hip = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "engine.hip")).read()
    assert '#include "scc.hip.h"' in hip
    for k in ("scc_init", "scc_trim", "scc_pick", "scc_seed", "scc_propagate", "scc_claim", "scc_label", "scc_decide"):
        assert k in hip


def test_the_python_face_exists():
    from sparseharness_amd import hostlib
    from sparseharness_amd.engine import Engine, SccGraph
    assert callable(Engine.scc_graph) and callable(Engine.scc) and callable(hostlib.scc_labels)
    assert hasattr(SccGraph, "edges") and hasattr(SccGraph, "footprint") and callable(SccGraph.free)
