"""The handle of Engine.bc_graph / Engine.betweenness.  It stands in a module of its own because tests/test_abi.py pins
the set of handle classes engine.py defines; tests/test_bc_abi.py makes the same checks of its bindings (every C function
it looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from .engine import _getter, _Graph


class BcGraph(_Graph):
    """What Engine.betweenness walks: the simple directed graph under the entries of a square matrix as in-lists and
    out-lists, both strictly ascending, with the level, sigma and delta of a source and the order array that is its queue
    (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_bc_graph"
    edges = _getter("edges", C.c_int64, "The edges of the simple directed graph (no self-loops, parallel entries once).")
    max_list = _getter("max_list", C.c_int64, "The length of the longest in- or out-list.")
