"""The reference of sh_tri (tests/tri_ref.py) against closed forms, and the host gold hostlib.triangle_counts against the
reference on every maker, on R-MAT-12 and on the golden matrices.  No GPU needed."""
import glob
import os
import re
from math import comb

import numpy as np
import pytest

import tri_ref as T
from conftest import ROOT
from sparseharness_amd import hostlib as H


def test_class_constants_mirror_the_kernels():
    text = open(os.path.join(ROOT, "sparseharness_amd", "csrc", "tri.hip.h")).read()
    got = {k: int(re.search(r"constexpr int " + k + r" = (\d+);", text).group(1)) for k in ("TRI_SHORT", "TRI_WAVE", "TRI_CHUNK")}
    assert (got["TRI_SHORT"], got["TRI_WAVE"], got["TRI_CHUNK"]) == (T.SHORT, T.WAVE, T.CHUNK)
    assert T.CLASS_LENGTHS == (T.SHORT, T.SHORT + 1, T.WAVE, T.WAVE + 1, T.CHUNK, T.CHUNK + 1)
    assert T.CHUNK + 1 <= 2399   # no path is reachable only by a forward list longer than K_2400's


@pytest.mark.parametrize("n", [1, 2, 3, 9, 65, 300])
def test_complete_graph(n):
    tri, deg, m = T.counts(*T.complete(n))
    assert m == comb(n, 2) and (deg == n - 1).all() and (tri == comb(n - 1, 2)).all()
    assert int(tri.sum()) == 3 * comb(n, 3)


@pytest.mark.parametrize("side", [2, 7, 40, 60])   # (60 x 60 = 3600 vertices: the set-based branch)
def test_triangulated_grid(side):
    tri, deg, m = T.counts(*T.triangulated_grid(side))
    assert int(tri.sum()) == 3 * 2 * (side - 1) ** 2
    assert m == 2 * side * (side - 1) + (side - 1) ** 2


@pytest.mark.parametrize("k,hub", [(5, "first"), (5, "last"), (1500, "first"), (1500, "last")])
def test_friendship(k, hub):
    n, rp, ci, va = T.friendship(k, hub)
    tri, deg, m = T.counts(n, rp, ci, va)
    h = 0 if hub == "first" else n - 1
    assert m == 3 * k and tri[h] == k and deg[h] == 2 * k
    rest = np.delete(np.arange(n), h)
    assert (tri[rest] == 1).all() and (deg[rest] == 2).all()


def test_bipartite():
    tri, deg, m = T.counts(*T.bipartite(30, 50))
    assert m == 1500 and not tri.any() and sorted(set(deg.tolist())) == [30, 50]


def test_dense_and_set_branches_agree():
    n, rp, ci, va = T.pattern(700, 6000)
    dense = T.counts(n, rp, ci, va)
    old, T.DENSE_LIMIT = T.DENSE_LIMIT, 0
    try:
        sets = T.counts(n, rp, ci, va)
    finally:
        T.DENSE_LIMIT = old
    assert np.array_equal(dense[0], sets[0]) and np.array_equal(dense[1], sets[1]) and dense[2] == sets[2]
    assert dense[0].any()


def makers():
    base = T.pattern()
    sym = lambda rp, ci, va: T.from_pairs(len(rp) - 1, *T.pairs_of(len(rp) - 1, rp, ci, va))   # noqa: E731
    r12 = H.rmat(12)
    out = {
        "complete-65": T.complete(65), "friendship-first": T.friendship(400, "first"), "friendship-last": T.friendship(400, "last"),
        "bipartite": T.bipartite(40, 70), "grid": T.triangulated_grid(30), "one-way": T.one_way_triangles(),
        "pattern": base, "upper": T.upper_only(*base), "lower": T.lower_only(*base), "noise": T.with_noise(*base),
        "class-limits": T.class_limits(), "empty": (0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
        "rmat12": (1 << 12,) + r12, "rmat12-sym": sym(*r12),
    }
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "matrix*.npz"))):
        out[os.path.basename(path)] = path
    return out


MAKERS = makers()


def load_golden(path):
    z = np.load(path)
    rp, ci, va = z["f32_row_ptr"], z["f32_col_idx"], z["f32_val"]
    return len(rp) - 1, rp, ci, va


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_host_gold_equals_reference(name):
    g = MAKERS[name]
    n, rp, ci, va = load_golden(g) if isinstance(g, str) else g
    tri, deg, m = T.counts(n, rp, ci, va)
    got_tri, got_deg = H.triangle_counts(rp, ci, va)
    assert got_tri.dtype == np.uint64 and got_deg.dtype == np.int32
    assert np.array_equal(got_tri, tri) and np.array_equal(got_deg, deg)
    assert int(deg.sum()) == 2 * m


def test_storage_forms_and_noise_change_nothing():
    base = T.pattern()
    want = T.counts(*base)
    for form in (T.upper_only(*base), T.lower_only(*base), T.with_noise(*base)):
        got = T.counts(*form)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert T.counts(*T.noise_as_edges(*T.with_noise(*base)))[2] > want[2]   # (the noise would count if zeros did)
    assert int(T.counts(*T.one_way_triangles())[0].sum()) >= 3 * 400
