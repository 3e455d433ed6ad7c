"""The handle of Engine.rcm_graph / Engine.rcm_order.  It stands in a module of its own because tests/test_abi.py pins
the set of handle classes engine.py defines; tests/test_rcm_abi.py makes the same checks of its bindings (every C function
it looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from .engine import _getter, _Graph


class RcmGraph(_Graph):
    """What Engine.rcm_order orders: the simple undirected graph under the entries of a square matrix as symmetric lists
    over the vertices sorted by (degree, index), with the map back and the state of a call (made from the host CSR arrays
    alone; needs no CsrMatrix)."""
    _c = "sh_rcm_graph"
    edges = _getter("edges", C.c_int64, "M: the edges of the simple undirected graph.")
    max_degree = _getter("max_degree", C.c_int64, "The largest degree (the length of the longest list).")
