"""The handle of Engine.trsv_graph / Engine.trsv.  It stands in a module of its own because tests/test_abi.py pins the set
of handle classes engine.py defines; tests/test_trsv_abi.py makes the same checks of its bindings (every C function it
looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from . import abi
from .engine import _getter, _Graph

# trsv.hip.h's constants, which the plan of a call is a function of (tests/test_trsv_abi.py compares them with the source)
TRSV_RUN = 1024        # levels of one run at most
TRSV_THIN = 256        # the default `thin`
TRSV_THIN_MAX = 1 << 16


class TrsvGraph(_Graph):
    """What Engine.trsv solves with: one triangle of a square matrix as lists in ascending (column, position as given)
    with their float32 values, the float64 diagonal, and the level sets of the dependency graph (made from the host CSR
    arrays alone; needs no CsrMatrix)."""
    _c = "sh_trsv_graph"
    entries = _getter("entries", C.c_int64, "The list entries: strictly-triangular entries with a column inside the matrix.")
    edges = entries   # (what _Graph calls them)
    levels = _getter("levels", C.c_int64, "The level sets (0 for a matrix without rows).")
    max_list = _getter("max_list", C.c_int64, "The length of the longest list.")
    max_width = _getter("max_width", C.c_int64, "The rows of the widest level.")
    zero_diag = _getter("zero_diag", C.c_int64, "The rows whose diagonal d is zero or missing (always 0 when unit).")
    first_zero = _getter("first_zero", C.c_int64, "The smallest such row, -1 if there is none.")

    def level(self, vec):
        """level[r] into an int32 vector of >= rows elements: 0 for an empty list, else 1 + the largest level in r's list."""
        self.engine._chk(abi.load().sh_trsv_graph_level(self.engine.h, self.h, vec.h))
