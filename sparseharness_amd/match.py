"""The handle of Engine.match_graph / Engine.matching.  It stands in a module of its own because tests/test_abi.py pins
the set of handle classes engine.py defines; tests/test_match_abi.py makes the same checks of its bindings (every C
function it looks up by its prefix is in abi.SIGNATURES with the types it passes)."""
from .engine import _Graph


class MatchGraph(_Graph):
    """What Engine.matching searches: the edges of the simple undirected graph under the entries of a square matrix as a
    flat list (ends and the key of the lightest entry of each), with one 64-bit word per vertex and two work lists of edge
    ids (made from the host CSR arrays alone; needs no CsrMatrix).  G.edges is M."""
    _c = "sh_match_graph"
