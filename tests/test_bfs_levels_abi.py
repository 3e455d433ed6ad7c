"""The direction-optimising BFS -- sh_bfs_graph_create / _free / _footprint / _edges and sh_bfs_levels -- is declared in
include/sparseharness_hip.h with the agreed parameter lists, exported by the library and bound in abi.SIGNATURES with the
declared argument types; argument errors come back before any device is touched.  No compute is called here (no GPU needed)."""
import ctypes as C
import os

from abi_checks import HEADER, check_create_errors, check_entry_points, last_error, section_comment
from conftest import ROOT
from sparseharness_amd import abi

WANT = {
    "sh_bfs_graph_create": ["sh_engine *", "int64_t", "int64_t", "const int32_t *", "const int32_t *", "const void *",
                            "sh_bfs_graph * *"],
    "sh_bfs_graph_free": ["sh_engine *", "sh_bfs_graph *"],
    "sh_bfs_graph_footprint": ["const sh_bfs_graph *", "uint64_t *"],
    "sh_bfs_graph_edges": ["const sh_bfs_graph *", "int64_t *"],
    "sh_bfs_levels": ["sh_engine *", "sh_bfs_graph *", "const sh_vec *", "sh_vec *", "sh_vec *", "int32_t", "double", "double",
                      "int32_t *", "int64_t *", "int32_t *", "int32_t *", "int64_t *", "int64_t *", "uint64_t *", "uint64_t *"],
}


def test_bfs_entry_points_are_declared_exported_and_bound():
    check_entry_points(WANT)


def test_section_comment_cites_what_it_extends_and_what_it_leaves_out():
    comment = section_comment("typedef struct sh_bfs_graph sh_bfs_graph;")
    for cite in ("app/bfs.cpp:94-174", "inc/harness.h:149-195", "no counterpart", "NOT covered", "other semirings",
                 "sh_bits_iterate", "row pieces", "multi-GPU", "C++ harness apps", "up_share", "down_share",
                 "Measured on an MI355X", "Rule:", "sh_iterate"):
        assert cite in comment, cite


def test_footprint_formula_is_stated_in_the_header():
    """The formula tests/test_bfs_levels_gpu.py compares sh_bfs_graph_footprint with is the header's."""
    text = " ".join(open(HEADER).read().split())
    assert "8 * (rows + 1) + 8 * edges + 8 * rows + 8 * W + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 18432" in text
    assert "W = (rows + 31) / 32" in text


def levels(max_levels, up=-1.0, down=-1.0):
    d, r, c = C.c_int32(), C.c_int64(), C.c_int32()
    return abi.load().sh_bfs_levels(None, None, None, None, None, max_levels, up, down, C.byref(d), C.byref(r), C.byref(c),
                                    None, None, None, None, None)


def test_argument_errors_need_no_device():
    """Every argument error named in the header comes back with a message that names the argument before anything
    touches a device (without an engine the message is the thread's, as for sh_engine_create)."""
    lib = abi.load()
    check_create_errors("sh_bfs_graph_create")
    b, k = C.c_uint64(), C.c_int64()
    assert lib.sh_bfs_graph_footprint(None, C.byref(b)) == abi.SH_EINVAL
    assert lib.sh_bfs_graph_edges(None, C.byref(k)) == abi.SH_EINVAL
    assert lib.sh_bfs_graph_free(None, None) == abi.SH_OK   # (freeing nothing is fine, as sh_csr_free)
    for cap in (0, -3):
        assert levels(cap) == abi.SH_EINVAL and "max_levels" in last_error()
    assert levels(10, up=float("nan")) == abi.SH_EINVAL and "up_share" in last_error() and "NaN" in last_error()
    assert levels(10, down=float("nan")) == abi.SH_EINVAL and "down_share" in last_error() and "NaN" in last_error()
    assert levels(10) == abi.SH_EINVAL and "NULL" in last_error()
    assert levels(10, up=float("inf"), down=0.0) == abi.SH_EINVAL and "NULL" in last_error()   # (infinite shares are legal)


def test_resource_check_covers_the_bfs_kernels():
    src = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "check_resources.py")).read()
    for k in ("bfs_init", "bfs_topdown", "bfs_bottomup", "bfs_queue_from_bitmap", "bfs_decide", "bfs_parents",
              "frontier_mark", "msbfs_csr", "spmm_csr", "spmv_tiled"):
        assert k in src
    mk = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "Makefile")).read()
    assert "bfs.hip.h" in mk
