"""The handle of Engine.ilu0_graph / Engine.ilu0.  It stands in a module of its own because tests/test_abi.py pins the set
of handle classes engine.py defines; tests/test_ilu0_abi.py makes the same checks of its bindings (every C function it
looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from . import abi
from .engine import _getter, _Graph

# ilu0.hip.h's constants, which the plan and the tiers of a call are functions of (tests/test_ilu0_abi.py compares them
# with the source)
ILU0_RUN = 1024          # levels of one run at most
ILU0_THIN = 256          # the default `thin`
ILU0_THIN_MAX = 1 << 16
ILU0_LANE_WORK = 256     # look-ups of a row its lane eliminates alone at most (the sweep's choice: DESIGN.md 6r)


class Ilu0Graph(_Graph):
    """What Engine.ilu0 factorises with: the slots of a square pattern (the distinct columns of every row in ascending
    order), where every input position goes, and the level sets of the lower triangle's dependency graph (made from the
    host row_ptr / col_idx alone; needs no CsrMatrix and no values).  One handle serves any number of Engine.ilu0 calls
    with new values."""
    _c = "sh_ilu0_graph"
    entries = _getter("entries", C.c_int64, "The slots: distinct (row, column) pairs with a column inside the matrix.")
    edges = entries   # (what _Graph calls them)
    levels = _getter("levels", C.c_int64, "The level sets (0 for a matrix without rows).")
    max_list = _getter("max_list", C.c_int64, "The slots of the longest row.")
    max_width = _getter("max_width", C.c_int64, "The rows of the widest level.")
    missing_diag = _getter("missing_diag", C.c_int64, "The rows without a diagonal slot.")
    first_missing = _getter("first_missing", C.c_int64, "The smallest such row, -1 if there is none.")
    work = _getter("work", C.c_int64, "The look-ups of one factorisation: over every lower slot (r, k), the upper slots of row k.")

    def level(self, vec):
        """level[r] into an int32 vector of >= rows elements: 0 for a row without a lower slot, else 1 + the largest level
        among its lower slots (TrsvGraph(uplo=0).level of the same arrays)."""
        self.engine._chk(abi.load().sh_ilu0_graph_level(self.engine.h, self.h, vec.h))
