"""tests/color_ref.py is pinned here (no GPU): the model of the Jones-Plassmann schedule == the plain serial first-fit
in the order == the host gold (hostlib.greedy_colors), for the three orders, two seeds and a prio vector with ties; the
model's round sizes are the histogram of the gold's chain depths; every answer has the properties of a greedy
colouring; and the rules the kernels rest on do bite -- broken on purpose, the model gives a wrong or improper
colouring on a named small graph.  Every comparison is exact."""
import numpy as np
import pytest

import color_ref as K
import core_ref as R
import tri_ref as T
import wcc_ref as W
from sparseharness_amd import hostlib as H

MAKERS = {
    "path": lambda: W.path(50),
    "star": lambda: R.star(40),
    "K9": lambda: T.complete(9),
    "K10": lambda: T.complete(10),
    "K5+ear": K.ear,
    "wheel": K.wheel,
    "grid16": lambda: W.grid(16),
    "rmat10": lambda: (1 << 10,) + H.rmat(10, seed=40),
    "messy": K.messy,
}
_cache = {}


def matrix(name):
    if name not in _cache:
        n, rp, ci, va = MAKERS[name]()
        _cache[name] = (n, rp, ci, np.ascontiguousarray(va))
    return _cache[name]


def tied_prio(n):
    """Priorities in -2 .. 2 only: most pairs tie, and the tie of the order decides."""
    return (np.random.default_rng(11).integers(-2, 3, n)).astype(np.int32)


ORDERINGS = [(0, 0, False), (1, 0, False), (1, 12345, False), (2, 0, False), (2, 0xFFFFFFFF, False), (0, 0, True), (1, 7, True)]


@pytest.mark.parametrize("order,seed,with_prio", ORDERINGS)
@pytest.mark.parametrize("name", list(MAKERS))
def test_model_serial_loop_and_host_gold_agree(name, order, seed, with_prio):
    mat = matrix(name)
    n = mat[0]
    prio = tied_prio(n) if with_prio else None
    m = K.schedule(*mat, order=order, seed=seed, prio=prio)
    color, colors, depth = K.first_fit(*mat, order=order, seed=seed, prio=prio)
    gcolor, gcolors, gdepth = H.greedy_colors(*mat[1:], order=order, seed=seed, prio=prio)
    assert np.array_equal(m["color"], color) and np.array_equal(gcolor, color)
    assert m["colors"] == colors == gcolors
    assert np.array_equal(gdepth, depth)
    assert m["complete"] is True and m["coloured"] == n
    # round r's list is the vertices of chain depth r
    assert m["rounds"] == int(depth.max()) + 1
    assert np.array_equal(m["size"], np.bincount(gdepth, minlength=m["rounds"]))
    assert np.array_equal(m["edges"], np.bincount(gdepth, weights=m["deg"], minlength=m["rounds"]).astype(np.int64))
    # the colours do not depend on the window
    for window in (64, 128):
        w = K.schedule(*mat, order=order, seed=seed, prio=prio, window=window)
        assert np.array_equal(w["color"], color) and np.array_equal(w["size"], m["size"])
    # properties of a greedy colouring
    assert K.is_proper(*mat, color)
    assert (color <= m["wait"]).all()             # at most one colour per preceding neighbour is held
    assert colors <= m["max_degree"] + 1
    u, v = T.pairs_of(*mat)
    zero = color == 0
    assert not (zero[u] & zero[v]).any()          # class 0 is independent ...
    touched = np.zeros(n, bool)
    touched[u[zero[v]]] = True
    touched[v[zero[u]]] = True
    assert (zero | touched).all()                 # ... and maximal: every other vertex has a neighbour in it


def test_closed_forms():
    for n in (9, 10):
        m = K.schedule(*matrix(f"K{n}"), order=1, seed=3)
        assert m["colors"] == n and m["rounds"] == n and sorted(m["color"].tolist()) == list(range(n))
        assert (m["size"] == 1).all() and (m["edges"] == n - 1).all()
    p = K.schedule(*matrix("path"), order=0)      # the natural order on a path: one vertex per round
    assert p["rounds"] == 50 and p["colors"] == 2 and p["color"].tolist() == [0, 1] * 25
    s = K.schedule(*matrix("star"), order=2)
    assert s["rounds"] == 2 and s["color"][0] == 0 and (s["color"][1:] == 1).all()
    g = K.schedule(*matrix("grid16"), order=0)    # the anti-diagonals of the grid
    assert g["rounds"] == 31 and g["colors"] == 2


def test_cut_short():
    m = K.schedule(*matrix("path"), order=0, max_rounds=3)
    assert m["complete"] is False and m["coloured"] == 3 and m["rounds"] == 3
    assert m["color"][:3].tolist() == [0, 1, 0] and (m["color"][3:] == -1).all()


def test_broken_rules_give_wrong_colourings():
    """The rules of color.hip.h, broken one at a time on K_66 with windows of 64 colours (its last two vertices need a
    second window) and on K_9.
    Decrementing the coloured neighbours too is the one change that is harmless by itself: a coloured vertex's word is 0
    and is never read again, so the colours stay -- the kernel skips those decrements to save the atomics, and the
    model says so.  What does break: a walk per window that decrements every time (the vertex behind the one that
    walked twice is never released at exactly 0), marks taken from the first window only (two vertices share colour 64),
    and a tie that is no bijection (two neighbours neither of which precedes the other land in one list)."""
    k66 = T.complete(66)
    good = K.schedule(*k66, order=0, window=64)
    assert good["colors"] == 66 and K.is_proper(*k66, good["color"]) and good["complete"]
    same = K.schedule(*k66, order=0, window=64, decrement_coloured=True)
    assert np.array_equal(same["color"], good["color"]) and np.array_equal(same["size"], good["size"])
    bad = K.schedule(*k66, order=0, window=64, every_walk_decrements=True)
    assert not bad["complete"] and bad["coloured"] == 65 and bad["color"][65] == -1
    bad = K.schedule(*k66, order=0, window=64, first_window_only=True)
    assert not K.is_proper(*k66, bad["color"]) and bad["color"][64] == bad["color"][65] == 64
    k9 = matrix("K9")
    bad = K.schedule(*k9, order=1, seed=0, tie=lambda v: K.mix32(v).astype(np.int64) & 1)
    assert not K.is_proper(*k9, bad["color"])


def test_mix32_is_injective_on_small_words_and_matches_the_gold():
    words = K.mix32(np.arange(1 << 16))
    assert len(np.unique(words)) == 1 << 16
    assert int(K.mix32(np.array([0]))[0]) == 0   # (every step maps 0 to 0)
    # the gold's order 1 on a graph without edges colours everything 0; on K_n the colours are the ranks of the mixed
    # words, which pins the gold's mix32 against this one word for word
    n, seed = 64, 99
    gcolor, _, _ = H.greedy_colors(*T.complete(n)[1:], order=1, seed=seed)
    rank = np.argsort(np.argsort(-K.mix32(np.arange(n) ^ seed).astype(np.int64)))
    assert np.array_equal(gcolor, rank)
