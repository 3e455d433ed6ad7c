"""The reference of sh_bfs_levels: a numpy BFS written from the definition in include/sparseharness_hip.h (cross-checked
against scipy.sparse.csgraph in tests/test_bfs_levels_gpu.py) and the header's switching rule evaluated on it.  CPU only:
numpy and graph_patterns, nothing of the engine.  Not a test and not a conftest."""
import numpy as np

from graph_patterns import rows_of_entries

UP_DEFAULT, DOWN_DEFAULT = 0.005, 0.01   # what a negative share means (include/sparseharness_hip.h)


class Bfs:
    pass


def edges_of(n, rp, ci, va):
    """(c, r) of every edge c -> r: row r stores column c, 0 <= c < n, with a value whose 32 bits are not all zero."""
    keep = (np.ascontiguousarray(va).view(np.uint32) != 0) & (ci >= 0) & (ci < n)
    return ci[keep].astype(np.int64), rows_of_entries(rp)[keep].astype(np.int64)


def oracle_bfs(n, rp, ci, va, x0, max_levels=None):
    c, r = edges_of(n, rp, ci, va)
    b = Bfs()
    b.n, b.E = n, len(c)
    b.outdeg, b.indeg = np.bincount(c, minlength=n), np.bincount(r, minlength=n)
    level = np.full(n, -1, np.int32)
    frontier = np.asarray(x0) != 0
    level[frontier] = 0
    b.sizes, b.m, b.open_entries = [int(frontier.sum())], [int(b.outdeg[frontier].sum())], []
    L = 0
    while frontier.any() and (max_levels is None or L < max_levels):   # step L assigns level L + 1
        b.open_entries.append(int(b.indeg[level == -1].sum()))         # entries kept of the rows unvisited before the step
        new = np.zeros(n, bool)
        new[r[frontier[c]]] = True
        new &= level == -1
        level[new] = L + 1
        frontier = new
        b.sizes.append(int(new.sum()))
        b.m.append(int(b.outdeg[new].sum()))
        L += 1
    b.steps, b.complete = L, not frontier.any()
    b.level = level
    b.depth = int(level.max()) if n else 0
    b.depth = max(b.depth, 0)
    b.reached = int((level >= 0).sum())
    ok = (level[r] > 0) & (level[c] == level[r] - 1)
    parent = np.full(n, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(parent, r[ok], c[ok])
    parent[parent == np.iinfo(np.int32).max] = -1
    b.parent = parent.astype(np.int32)
    assert ((b.parent >= 0) == (level > 0)).all()
    return b


def predict_modes(b, up, down):
    """The switching rule of the header evaluated on the oracle's m_L and |F_L|."""
    if up < 0:
        up = UP_DEFAULT
    if down < 0:
        down = DOWN_DEFAULT
    modes, mode = [], 1 if b.m[0] > up * b.E else 0
    for L in range(b.steps):
        modes.append(mode)
        if mode == 0:
            mode = 1 if b.m[L + 1] > up * b.E else 0
        else:
            mode = 0 if b.sizes[L + 1] < down * b.n else 1
    return modes
