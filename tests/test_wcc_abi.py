"""sh_wcc -- sh_wcc_graph_create / _free / _footprint / _edges and sh_wcc -- is declared in include/sparseharness_hip.h
with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the declared argument types;
argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_wcc_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_wcc_graph * *"],
    "sh_wcc_graph_free": ["sh_engine *", "sh_wcc_graph *"],
    "sh_wcc_graph_footprint": ["const sh_wcc_graph *", "uint64_t *"],
    "sh_wcc_graph_edges": ["const sh_wcc_graph *", "int64_t *"],
    "sh_wcc": ["sh_engine *", "sh_wcc_graph *", "sh_vec *", "int32_t", "int32_t", "int64_t *", "int64_t *", "int32_t *",
               "int32_t *", "int32_t *", "int64_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}


def test_wcc_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_states_the_contract_and_what_it_leaves_out():
    comment = section_comment("typedef struct sh_wcc_graph sh_wcc_graph;")
    for cite in ("row r storing column c with 0 <= c < rows", "not all zero", "direction is ignored", "largest", "does not depend on",
                 "trees only", "No kernel ever waits", "Measured on an MI355X", "Rule:", "NOT covered", "multi-GPU", "row pieces",
                 "C++ harness apps", "component sizes", "histogram", "incremental updates", "max_rounds", "sample"):
        assert cite in comment, cite
    assert "@" not in comment   # no placeholder left where the measurements go


def test_scc_section_points_here():
    """Weakly connected components are no longer among what sh_scc's section lists as not covered without a pointer."""
    comment = section_comment("typedef struct sh_scc_graph sh_scc_graph;")
    assert "sh_wcc" in comment and "6h" in comment


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_wcc_gpu.py compares sh_wcc_graph_footprint with is the header's."""
    text = " ".join(section_comment("typedef struct sh_wcc_graph sh_wcc_graph;").split())
    assert "8 * (rows + 1) + 8 * edges + 8 * rows + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 34816" in text


def wcc(sample, max_rounds):
    k, s, r, c = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
    return abi.load().sh_wcc(None, None, None, sample, max_rounds, C.byref(k), C.byref(s), C.byref(r), C.byref(c),
                             None, None, None, None, None, None)


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_wcc_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_wcc_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_wcc_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_wcc_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    for s in (-1, -7):
        assert wcc(s, 10) == abi.SH_EINVAL and "sample" in last_error()
    for cap in (0, -3):
        assert wcc(2, cap) == abi.SH_EINVAL and "max_rounds" in last_error()
    assert wcc(2, 10) == abi.SH_EINVAL and "NULL" in last_error() and "comp" in last_error()
    assert wcc(0, 1) == abi.SH_EINVAL and "NULL" in last_error()   # (sample = 0 and max_rounds = 1 are legal)


def test_resource_check_covers_the_wcc_kernels():
    kernels = ("wcc_init", "wcc_sample", "wcc_compact", "wcc_full", "wcc_jump", "wcc_decide", "wcc_label")
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in kernels + ("scc_trim", "sssp_relax", "bfs_topdown", "frontier_mark"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "wcc.hip.h" in mk
    hip = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "engine.hip")).read()
    assert '#include "wcc.hip.h"' in hip
    for k in kernels:
        assert k in hip
    code = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "wcc.hip.h")).read()
    for phrase in ("TREES ONLY EVER MERGE", "NO LIST CAN OVERFLOW", "NO KERNEL EVER WAITS"):
        assert phrase in code


def test_the_python_face_exists():
    import inspect

    from sparseharness_amd import hostlib
    from sparseharness_amd.engine import Engine, WccGraph
    assert callable(Engine.wcc_graph) and callable(Engine.wcc) and callable(hostlib.wcc_labels)
    assert hasattr(WccGraph, "edges") and hasattr(WccGraph, "footprint") and callable(WccGraph.free)
    sig = inspect.signature(Engine.wcc)
    assert sig.parameters["sample"].default == 2 and sig.parameters["max_rounds"].default == 1 << 20
