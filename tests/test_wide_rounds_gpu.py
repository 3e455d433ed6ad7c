"""Every worklist driver on one input whose rounds are wider than a traversal launch: tri_ref.friendship(300_000), a hub
tied to 600 000 leaves that are tied in pairs (600 001 vertices, 900 000 edges, 300 000 triangles).

A traversal launch is at most 1024 workgroups of 256 threads, and a workgroup leaves its sums in one part.  Only a round
of more than 1024 * 256 = 262 144 list entries gives the last workgroup a part that is not zero and all four strides of
the closing fold something to carry; the other GPU tests top out at 32 768 vertices and one hub of 70 001, so a fold that
dropped a wave, a stride or the last parts would pass them.  Here each driver is compared with its own reference, as in
its test_*_gpu.py (whose run / check / same / want are used, not copied): every output vector, every scalar and every
per-round record with ==.  Where the reference has per-round sizes the test first asserts that its largest round is
wider than 262 144, so that it cannot lose its point silently."""
import numpy as np
import pytest

import core_ref
import minplus_ref
import scc_ref
import test_bfs_levels_gpu as bfs
import test_color_gpu as color
import test_core_gpu as core
import test_match_gpu as match
import test_msf_gpu as msf
import test_rcm_gpu as rcm
import test_scc_gpu as scc
import test_sssp_gpu as sssp
import test_tri_gpu as tri
import test_truss_gpu as truss
import test_wcc_gpu as wcc
import tri_ref
import truss_ref
import wcc_ref
from guarded import _not_halted   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd.engine import Engine

pytestmark = pytest.mark.gpu

K = 300_000
NAME = "friendship300k"
LAUNCH = 1024 * 256   # list entries one traversal launch takes in one stride
_mat = []


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def wide():
    """(n, row_ptr, col_idx, values), built once and never written to."""
    if not _mat:
        n, rp, ci, va = tri_ref.friendship(K)
        va = np.ascontiguousarray(va)
        for a in (rp, ci, va):
            a.setflags(write=False)
        _mat.append((n, rp, ci, va))
        assert n == 2 * K + 1 and len(ci) == 6 * K
    return _mat[0]


def frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def test_bfs_levels(eng):
    n, rp, ci, va = wide()
    x0 = bfs.source_vector(n, [0])
    b = bfs.oracle_bfs(n, rp, ci, va, x0)
    assert max(b.sizes) > LAUNCH and b.sizes[:2] == [1, 2 * K]
    G = eng.bfs_graph(rp, ci, va)
    try:
        assert G.edges == b.E
        for shares in (bfs.TOP_DOWN, bfs.BOTTOM_UP, bfs.DEFAULT):
            level, parent, res = bfs.run(eng, G, x0, shares)
            bfs.check(b, level, parent, res, shares, NAME)
    finally:
        G.free()


def test_sssp(eng):
    mat = wide()
    n, rp, ci, va = mat
    x0 = minplus_ref.start_vector(n, 0)
    # from the input alone: the source is the hub, every other vertex is in its list and one weight away, so under any
    # bucket width the round after the hub's relaxes from all 2K of them
    assert int(rp[1] - rp[0]) == 2 * K > LAUNCH and (va == 1.0).all()
    want_dist = sssp.reference(NAME, x0, mat)[0]
    assert want_dist[0] == 0.0 and (want_dist[1:] == 1.0).all()
    G = eng.sssp_graph(rp, ci, va)
    try:
        for delta in (-1.0, float("inf")):
            dist, pred, res = sssp.run(eng, G, x0, delta)
            sssp.check(NAME, x0, dist, pred, res, f"delta {delta}", mat=mat)
            assert int(res[5].max()) == 2 * K > LAUNCH   # the near list of the round after the hub's
    finally:
        G.free()


def test_scc(eng):
    mat = wide()
    ref = scc_ref.components(*mat)
    scheds = {(t, p): scc_ref.schedule(*mat, t, p) for t, p in scc.SETTINGS}
    assert all(max(s[2]) > LAUNCH for s in scheds.values()) and (ref == mat[0] - 1).all()   # one component of 600 001
    scc.components_and_rounds_under_every_setting(eng, NAME, mat, ref, lambda trim, pivot: scheds[(trim, pivot)])


def test_wcc(eng):
    mat = wide()
    ref = wcc_ref.components(*mat)
    ref.setflags(write=False)
    # from the input alone: every row holds an entry, so sampling round 0 looks at one entry per row, and a call without
    # sampling walks every stored entry in its first round; either is wider than a launch
    n, rp, ci, va = mat
    assert (np.diff(rp) >= 1).all() and n > LAUNCH and len(ci) > LAUNCH and (ref == n - 1).all()
    out = wcc.check(eng, NAME, mat=mat, ref=ref)
    for sample, res in out.items():
        edges = res[7]
        assert int(edges.max()) > LAUNCH, sample   # entries walked by its widest round


def test_tri(eng):
    mat = wide()
    w = tri_ref.counts(*mat)
    assert w[2] == 3 * K and int(w[0].sum()) == 3 * K
    # order = 1 only: under it every forward list has at most two entries and every workgroup of tri_count_light leaves a
    # part.  Under order = 0 the hub's forward list holds all 600 000 leaves and ONE workgroup walks it once per chunk of
    # 2048 (47 s, measured): that is the heavy class's worst case, which test_tri_gpu.py covers at its own sizes, not a fold.
    total, probes, longest = tri.check(eng, NAME, 1, mat=mat, w=w)
    assert total == K and longest == 2


def test_core(eng):
    mat = wide()
    w = frozen(core_ref.peel(*mat))
    assert int(w["size"].max()) > LAUNCH
    for chase in core.CHASES:
        core.check(eng, NAME, chase, mat=mat, w=w)


def test_truss(eng):
    mat = wide()
    w = frozen(truss_ref.peel(*mat))
    assert int(w["size"].max()) > LAUNCH and w["triangles"] == K
    truss.check(eng, NAME, mat=mat, w=w)


def test_color(eng):
    mat = wide()
    w = color.want(NAME, 2, 0, mat=mat)
    assert int(w["size"].max()) > LAUNCH and w["colors"] == 3   # (the largest colour is folded by a maximum)
    got = color.run(eng, mat, 2, 0)
    color.same(got, w, mat[0])
    assert got["complete"] is True and got["coloured"] == mat[0] and int(got["size"].sum()) == mat[0]


def test_msf(eng):
    mat = wide()
    w = msf.want(NAME, mat=mat)
    assert int(w["walked"].max()) > LAUNCH and int(w["hooks"].max()) > LAUNCH
    got = msf.run(eng, mat)
    msf.same(got, w, mat[0])
    assert got["complete"] is True and int(got["in_msf"].sum()) == got["tree_edges"] == mat[0] - got["components"]


def test_match(eng):
    mat = wide()
    w = match.want(NAME, 1, 1, mat=mat)
    assert int(w["walked"].max()) > LAUNCH
    got = match.run(eng, mat, 1, 1)
    match.same(got, w, mat[0])
    assert got["complete"] is True and int(got["in_match"].sum()) == got["pairs"] == int((got["mate"] >= 0).sum()) // 2


def test_rcm(eng):
    mat = wide()
    w = rcm.want(NAME, mat=mat)
    assert int(w["size"].max()) > LAUNCH and w["profile_before"] > 1 << 32   # (the 64-bit sum is exercised)
    got = rcm.run(eng, mat)
    rcm.same(got, w, mat[0])
    assert got["complete"] is True and np.array_equal(got["perm"][got["pos"]], np.arange(mat[0]))
