"""sh_bc on the GPU: bc and sigma as float64 bit patterns, level, and the per-source figures against tests/bc_ref.py's
ordered (pinned by tests/test_bc_ref.py) and, on the shapes Python cannot afford, against the host gold (which the same
file pins against ordered bit for bit).  The cases are tests/bc_ref.py's CASES; "graphs4" is all 4096 digraphs of 4
vertices side by side, every vertex a source.

Every comparison is exact (==): the header fixes the order of every addition as a function of the list alone, and every
value has one owner, whatever the lanes race on.  (The one exception is written into the header: once sigma has
overflowed, inf / inf is a NaN whose sign and payload IEEE leaves open; there a NaN must stand where a NaN stands.)  The
shapes are the smallest at which a kernel can still go wrong: lists on both sides of the tiers of the sum (one lane up to
BC_LANE entries, one wave up to BC_PIECE, several pieces beyond) and of a wave's stride (64), a level wider than a launch
has lanes, more steps than the first two batches hold, sigma exact, rounded and overflowed."""
import numpy as np
import pytest

import bc_ref as B
import guarded as GD
from guarded import _not_halted   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

BC_LANE, BC_PIECE, BC_MAX_BLOCKS = (B.constants()[k] for k in ("BC_LANE", "BC_PIECE", "BC_MAX_BLOCKS"))
CASES, case, want, header_footprint = B.CASES, B.case, B.want, B.header_footprint   # (shared with tests/test_bc_ref.py)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def run(eng, mat, sources, accumulate=0, start=None, G=None):
    """-> dict of one call's outputs (on a handle of its own unless G is given)."""
    n = mat[0]
    own = G is None
    if own:
        G = eng.bc_graph(*mat[1:])
    first = np.full(max(n, 1), -3.5) if start is None else np.asarray(start, np.float64)
    bc, sigma = eng.vector(first.view(np.uint32)), eng.vector(np.full(max(n, 1), -3.5).view(np.uint32))
    level = eng.vector(np.full(max(n, 1), 7, np.int32))
    try:
        steps, depth, reached, smax, edges, ns, total = GD.call(eng.betweenness, G, sources, bc, accumulate, sigma, level)
        out = dict(bc=bc.download(np.uint32, 2 * n).view(np.float64), sigma=sigma.download(np.uint32, 2 * n).view(np.float64),
                   level=level.download(np.int32, n), depth=depth, reached=reached, sigma_max=smax, edges=edges, steps=steps,
                   ns=ns, total=total, M=G.edges, max_list=G.max_list, footprint=G.footprint)
        return out
    finally:
        for v in (bc, sigma, level):
            v.free()
        if own:
            G.free()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, w, nan_ok=False, what=""):
    for f in ("bc", "sigma", "sigma_max"):
        g, x = np.asarray(got[f], np.float64), np.asarray(w[f], np.float64)
        if nan_ok:
            assert np.array_equal(np.isnan(g), np.isnan(x)), (what, f)
            g, x = np.where(np.isnan(g), 0.0, g), np.where(np.isnan(x), 0.0, x)
        bad = np.nonzero(bits(g) != bits(x))[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:5].tolist(), g[bad[:5]].tolist(), x[bad[:5]].tolist())
    for f in ("level", "depth", "reached", "edges"):
        assert np.array_equal(got[f], w[f]), (what, f)


# ---- 1. against the references
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_reference_bit_for_bit(eng, name):
    mat, sources = case(name)
    w = want(name)
    got = run(eng, mat, sources)
    same(got, w, nan_ok=name == "diamonds1030", what=name)
    ins, outs = B.lists(mat) if mat[0] < 20_000 else (None, None)
    if ins is not None:
        assert got["M"] == sum(len(x) for x in ins)
        assert got["max_list"] == max([len(x) for x in ins] + [len(x) for x in outs])
    assert got["footprint"] == header_footprint(mat[0], got["M"])
    assert got["steps"] == int((w["depth"] + 1).sum()) and len(got["ns"]) == len(sources)


def test_no_rows_and_one_row(eng):
    got = run(eng, B.csr(0, []), [])
    assert got["steps"] == 0 and got["M"] == 0 and got["footprint"] == header_footprint(0, 0)
    one = B.csr(1, [])
    for sources in ([], [0], [0, 0]):
        got = run(eng, one, sources)
        assert got["bc"].tolist() == [0.0] and got["M"] == 0 and got["footprint"] == header_footprint(1, 0)
        assert got["depth"].tolist() == [0] * len(sources) and got["reached"].tolist() == [1] * len(sources)
        # without sources sigma and level are left alone
        assert got["level"].tolist() == ([0] if sources else [7]) and got["sigma"].tolist() == ([1.0] if sources else [-3.5])
    # a self-loop and a stored zero are no edges
    n, rp, ci, _ = B.csr(2, [(0, 0), (0, 1)])
    got = run(eng, (n, rp, ci, np.array([1.0, 0.0], np.float32)), [0])
    assert got["M"] == 0 and got["reached"].tolist() == [1]


# ---- 2. schedule-freedom
@pytest.mark.parametrize("name", ("rmat10", "edges0", "K7,9"))
def test_the_same_call_twice_and_the_sources_one_call_each(eng, name):
    mat, sources = case(name)
    w = want(name)
    G = eng.bc_graph(*mat[1:])
    try:
        for _ in range(2):
            same(run(eng, mat, sources, G=G), w, what=name)
        bc = np.zeros(mat[0])
        for s in sources:   # one call per source, accumulate = 1: the bits of one call
            got = run(eng, mat, [s], accumulate=1, start=bc, G=G)
            bc = got["bc"].copy()
        assert np.array_equal(bits(bc), bits(w["bc"]))
        assert np.array_equal(bits(got["sigma"]), bits(w["sigma"])) and np.array_equal(got["level"], w["level"])
    finally:
        G.free()


@pytest.mark.parametrize("name", ("rmat10", "diamonds33", "star65-all"))
def test_the_stored_order_and_stored_duplicates_change_nothing(eng, name):
    mat, sources = case(name)
    w = want(name)
    for other in (B.restored(mat, reverse=True), B.restored(mat, twice=True)):
        assert not np.array_equal(other[2], mat[2])
        same(run(eng, other, sources), w, what=name)


# ---- 3. the per-source figures
@pytest.mark.parametrize("name", ("rmat10", "dead-end", "path100"))
def test_depth_and_reached_are_those_of_bfs_levels(eng, name):
    mat, sources = case(name)
    n = mat[0]
    got = run(eng, mat, sources)
    G = eng.bfs_graph(*mat[1:])
    try:
        for i, s in enumerate(sources):
            x0 = np.zeros(n, np.int32)
            x0[s] = 1
            xv, lv = eng.vector(x0), eng.alloc(n)
            depth, reached = GD.call(eng.bfs_levels, G, xv, lv)[:2]
            assert (depth, reached) == (got["depth"][i], got["reached"][i]), (name, s)
            if i == len(sources) - 1:
                assert np.array_equal(lv.download(np.int32, n), got["level"])
            xv.free(), lv.free()
    finally:
        G.free()
    assert np.array_equal(got["edges"], want(name)["edges"])


# ---- 4. the buffers
def test_only_the_stated_elements_change_and_argument_errors_leave_the_buffers_alone(eng):
    mat, sources = case("K7,9")
    n, w = mat[0], want("K7,9")
    lib = abi.load()
    dev = GD.Dev(lib, eng.h)
    G = eng.bc_graph(*mat[1:])
    spare = 6
    fill = np.full(2 * n + spare, 7, np.int32)
    bc, sigma = dev.guarded(fill, offset=2), dev.guarded(fill, offset=4)
    level = dev.guarded(fill[:n + spare], offset=1)
    odd, short, short_level = dev.guarded(fill, offset=1), dev.guarded(fill[:2 * n - 1], offset=0), dev.guarded(fill[:n - 1], offset=0)
    try:
        GD.call(eng.betweenness, G, sources, bc, 0, sigma, level)
        for v, f, k in ((bc, "bc", 2 * n), (sigma, "sigma", 2 * n), (level, "level", n)):
            got = v.read(f)
            assert (got[k:] == 7).all(), f
            want_bits = np.ascontiguousarray(w[f]).view(np.uint32)
            assert np.array_equal(got[:k], want_bits), f
        for v in (bc, sigma):
            dev.ok(lib.sh_vec_upload(eng.h, v.v, GD.vp(fill), len(fill)))
        bad_calls = (
            (dict(accumulate=2), abi.SH_EINVAL, "accumulate"),
            (dict(sources=[0, n]), abi.SH_EINVAL, "sources[1]"),
            (dict(sources=[-1]), abi.SH_EINVAL, "sources[0]"),
            (dict(bc=short), abi.SH_ESHAPE, "bc"),
            (dict(sigma=short), abi.SH_ESHAPE, "sigma"),
            (dict(level=short_level), abi.SH_ESHAPE, "level"),
            (dict(bc=odd), abi.SH_EINVAL, "aligned"),
            (dict(sigma=odd), abi.SH_EINVAL, "aligned"),
            (dict(sigma=bc), abi.SH_EINVAL, "alias"),
        )
        for change, code, word in bad_calls:
            args = dict(sources=sources, bc=bc, accumulate=0, sigma=sigma, level=None)
            args.update(change)
            with pytest.raises(EngineError) as err:
                eng.betweenness(G, **args)
            assert err.value.code == code and word in str(err.value) and "sh_bc" in str(err.value), (change, str(err.value))
        for v in (bc, sigma, odd):
            assert (v.read("after the refused calls") == 7).all()
    finally:
        for v in (bc, sigma, level, odd, short, short_level):
            v.free()
        G.free()
