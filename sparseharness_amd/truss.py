"""The handle of Engine.truss_graph / Engine.truss_numbers.  It stands in a module of its own because tests/test_abi.py
pins the set of handle classes engine.py defines; tests/test_truss_abi.py makes the same checks of its bindings (every C
function it looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from .engine import _getter, _Graph


class TrussGraph(_Graph):
    """What Engine.truss_numbers peels: the simple undirected graph under the entries of a square matrix as symmetric
    ascending lists with the edge id of every entry, the ends of every edge, the remaining supports and stamps of a call
    and two work lists (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_truss_graph"
    edges = _getter("edges", C.c_int64, "M: the edges of the simple undirected graph.")
    max_degree = _getter("max_degree", C.c_int64, "The largest degree (the length of the longest list).")
