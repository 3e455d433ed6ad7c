"""The handle of Engine.color_graph / Engine.greedy_colors.  It stands in a module of its own because tests/test_abi.py
pins the set of handle classes engine.py defines; tests/test_color_abi.py makes the same checks of its bindings (every C
function it looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
import ctypes as C

from .engine import _getter, _Graph


class ColorGraph(_Graph):
    """What Engine.greedy_colors colours: the simple undirected graph under the entries of a square matrix as symmetric
    ascending lists, with its degrees, the waiting counts of a call and two work lists (made from the host CSR arrays
    alone; needs no CsrMatrix)."""
    _c = "sh_color_graph"
    edges = _getter("edges", C.c_int64, "M: the edges of the simple undirected graph.")
    max_degree = _getter("max_degree", C.c_int64, "The largest degree (the length of the longest list).")
