"""sh_trsv on the GPU: x as float64 (or float32) bit patterns, level and the handle's figures against tests/trsv_ref.py's
restatement (pinned against the host gold and the exact rounding bound by tests/test_trsv_ref.py), and the plan of every
call against the restated plan.  The cases are tests/trsv_ref.py's CASES.

Every comparison is exact (==): the header fixes the order of every addition as a function of the list alone and every
x[r] has one owner; the one exception is written into the header: a NaN must stand where a NaN stands.  The shapes are the
smallest at which a kernel can still go wrong: lists on both sides of the tiers of the sum (one lane up to TRSV_LANE
entries, one wave up to TRSV_PIECE, several pieces beyond) and of a wave's stride (64), a level wider than a capped launch
has lanes, more levels than the analysis' first two batches hold, runs cut at TRSV_RUN, levels on both sides of `thin`."""
import ctypes as C

import numpy as np
import pytest

import guarded as GD
import trsv_ref as T
from guarded import _not_halted   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu

FIGURES = ("entries", "levels", "max_list", "max_width", "zero_diag", "first_zero")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def handle(eng, c):
    return eng.trsv_graph(*c["mat"][1:], c["uplo"], c["unit"])


def solve(eng, G, n, b, f32=0, thin=None, inplace=False):
    """-> (x, (launches, runs, levels_in_runs)) of one call on handle G."""
    dt = np.float32 if f32 else np.float64
    host = np.zeros(max(n, 1), dt)
    host[:n] = np.asarray(b, dt)[:n]
    bv = eng.vector(host.view(np.uint32))
    xv = bv if inplace else eng.vector(np.full(max(n, 1), -3.5, dt).view(np.uint32))
    try:
        launches, runs, in_runs, total = GD.call(eng.trsv, G, bv, xv, f32, thin)
        x = xv.download(np.uint32, (1 if f32 else 2) * n).view(dt)
        if not inplace:   # b is read only
            assert np.array_equal(bv.download(np.uint32, host.view(np.uint32).size), host.view(np.uint32))
        return x, (launches, runs, in_runs)
    finally:
        bv.free()
        if not inplace:
            xv.free()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_x(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what   # a NaN stands where a NaN stands
    ok = ~np.isnan(want)
    bad = np.nonzero(bits(got)[ok] != bits(want)[ok])[0]
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[ok][bad[:5]].tolist(), want[ok][bad[:5]].tolist())


# ---- 1. against the restatement: float64, float32, in place, the figures, the footprint, the levels, the default plan
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_equals_the_restatement_bit_for_bit(eng, name):
    c, w = T.case(name), T.want(name)
    n = c["mat"][0]
    G = handle(eng, c)
    lv = eng.vector(np.full(max(n, 1), 7, np.int32))
    try:
        assert {k: getattr(G, k) for k in FIGURES} == {k: w[k] for k in FIGURES}, name
        assert G.edges == w["entries"] and G.footprint == T.header_footprint(n, w["entries"], w["levels"])
        G.level(lv)
        assert np.array_equal(lv.download(np.int32, n), w["level"]), name
        x, plan = solve(eng, G, n, c["b"])
        same_x(x, w["x"], name)
        assert plan == T.plan(w["lstart"]), name
        x, _ = solve(eng, G, n, c["b"], inplace=True)
        same_x(x, w["x"], name + " in place")
        w32 = T.want(name, 1)
        for inplace in (False, True):
            x, plan = solve(eng, G, n, c["b"], f32=1, inplace=inplace)
            same_x(x, w32["x"], name + " f32")
            assert plan == T.plan(w["lstart"]), name
    finally:
        lv.free()
        G.free()


def test_no_rows_launch_nothing(eng):
    c = T.case("rows0")
    G = handle(eng, c)
    try:
        assert solve(eng, G, 0, c["b"])[1] == (0, 0, 0) and G.levels == 0 and G.footprint == T.header_footprint(0, 0, 0)
    finally:
        G.free()


# ---- 2. the plan and thin: x does not depend on it
@pytest.mark.parametrize("name", ("widths64", "widths256", "path-runs", "tiers"))
def test_the_plan_is_the_restated_one_and_x_does_not_depend_on_thin(eng, name):
    c, w = T.case(name), T.want(name)
    n = c["mat"][0]
    G = handle(eng, c)
    try:
        for thin in (0, 1, 64, None, n):
            x, plan = solve(eng, G, n, c["b"], thin=thin)
            same_x(x, w["x"], (name, thin))
            assert plan == T.plan(w["lstart"], thin), (name, thin)
    finally:
        G.free()
    if name == "path-runs":   # runs are cut at the cap: 1024 + 1024 + 3 levels
        assert T.plan(w["lstart"]) == (3, 3, 2 * T.RUN + 3)
    if name == "widths64":
        assert T.plan(w["lstart"], 64) == (4, 2, 3)


# ---- 3. handles
def test_two_handles_of_one_ilu_matrix_used_alternately_and_reused(eng):
    lo, up = T.case("ilu-lower-unit"), T.case("ilu-upper")
    mat, n = lo["mat"], lo["mat"][0]
    assert up["mat"] is not mat and np.array_equal(up["mat"][3], mat[3])   # (the same matrix, built twice)
    GL, GU = handle(eng, lo), handle(eng, up)
    try:
        rng = np.random.default_rng(9)
        for k in range(3):
            b = rng.normal(size=n)
            y, _ = solve(eng, GL, n, b)
            x, _ = solve(eng, GU, n, y)
            wy = T.solve(mat, b, 0, 1)["x"]
            same_x(y, wy, ("L", k))
            same_x(x, T.solve(mat, wy, 1, 0)["x"], ("U", k))
    finally:
        GL.free()
        GU.free()


def test_with_sh_color_the_levels_are_at_most_the_colours(eng):
    """The lower triangle of a 32 x 32 grid Laplacian, permuted by sh_color's classes (stable by colour): rows of one colour
    have no entry that couples them, so they share a level."""
    full = T.grid_lower(32)
    n = full[0]
    CG = eng.color_graph(*full[1:])
    cv = eng.vector(np.full(n, -1, np.int32))
    try:
        colors = GD.call(eng.greedy_colors, CG, cv)[0]
        color = cv.download(np.int32, n)
    finally:
        cv.free()
        CG.free()
    perm = np.argsort(color, kind="stable")
    mat = T.permuted(full, perm)
    b = np.random.default_rng(11).normal(size=n)
    w = T.solve(mat, b)
    G = eng.trsv_graph(*mat[1:])
    try:
        assert G.levels == w["levels"] <= colors and G.levels < T.solve(full, b)["levels"]
        same_x(solve(eng, G, n, b)[0], w["x"], "coloured grid")
    finally:
        G.free()


# ---- 4. the buffers and the refusals
def test_only_the_stated_elements_change_and_argument_errors_leave_the_buffers_alone(eng):
    c, w, w32 = T.case("ilu-upper"), T.want("ilu-upper"), T.want("ilu-upper", 1)
    n = c["mat"][0]
    lib = abi.load()
    dev = GD.Dev(lib, eng.h)
    G = handle(eng, c)
    spare = 6
    fill = np.full(2 * n + spare, 7, np.int32)
    b64 = np.full(2 * n + spare, 7, np.int32)
    b64[:2 * n] = np.asarray(c["b"], np.float64).view(np.int32)
    b32 = np.full(n + spare, 7, np.int32)
    b32[:n] = np.asarray(c["b"], np.float32).view(np.int32)
    b, x = dev.guarded(b64, offset=2), dev.guarded(fill, offset=4)
    bf, xf = dev.guarded(b32, offset=1), dev.guarded(fill[:n + spare], offset=3)
    odd, short, short32 = dev.guarded(fill, offset=1), dev.guarded(fill[:2 * n - 1], offset=0), dev.guarded(fill[:n - 1], offset=0)
    lv, short_lv = dev.guarded(fill[:n + spare], offset=1), dev.guarded(fill[:n - 1], offset=0)
    try:
        GD.call(eng.trsv, G, b, x)
        got = x.read("x")
        assert (got[2 * n:] == 7).all() and np.array_equal(got[:2 * n], w["x"].view(np.uint32))
        assert np.array_equal(b.read("b"), b64.view(np.uint32))
        GD.call(eng.trsv, G, bf, xf, 1)
        got = xf.read("x f32")
        assert (got[n:] == 7).all() and np.array_equal(got[:n], w32["x"].view(np.uint32))
        G.level(lv)
        got = lv.read("level")
        assert (got[n:] == 7).all() and np.array_equal(got[:n].view(np.int32), w["level"])
        dev.ok(lib.sh_vec_upload(eng.h, x.v, GD.vp(fill), len(fill)))
        overlap = eng.wrap(lib.sh_vec_device_ptr(b.v) + 8, 2 * n)
        bad_calls = (
            (dict(f32=2), abi.SH_EINVAL, "f32"),
            (dict(thin=T.THIN_MAX + 1), abi.SH_EINVAL, "thin"),
            (dict(b=short), abi.SH_ESHAPE, "b holds"),
            (dict(x=short), abi.SH_ESHAPE, "x holds"),
            (dict(b=short32, f32=1), abi.SH_ESHAPE, "b holds"),
            (dict(x=short32, f32=1), abi.SH_ESHAPE, "x holds"),
            (dict(b=odd), abi.SH_EINVAL, "aligned"),
            (dict(x=odd), abi.SH_EINVAL, "aligned"),
            (dict(x=overlap), abi.SH_EINVAL, "overlap"),
        )
        for change, code, word in bad_calls:
            args = dict(b=b, x=x, f32=0, thin=None)
            args.update(change)
            with pytest.raises(EngineError) as err:
                eng.trsv(G, **args)
            assert err.value.code == code and word in str(err.value) and "sh_trsv" in str(err.value), (change, str(err.value))
        with pytest.raises(EngineError) as err:
            G.level(short_lv)
        assert err.value.code == abi.SH_ESHAPE and "level" in str(err.value)
        overlap.free()
        assert (x.read("after the refused calls") == 7).all() and (odd.read("odd") == 7).all()
        assert np.array_equal(b.read("b after the refused calls"), b64.view(np.uint32))
        for bad in (dict(uplo=2), dict(uplo=-1), dict(unit=2)):
            with pytest.raises(EngineError) as err:
                eng.trsv_graph(*c["mat"][1:], **bad)
            assert err.value.code == abi.SH_EINVAL and list(bad)[0] in str(err.value)
        # an odd float32 offset is fine: only float64 vectors must be 8-byte aligned
        GD.call(eng.trsv, G, bf, xf, 1, 0)
        assert np.array_equal(xf.read("x f32 again")[:n], w32["x"].view(np.uint32))
    finally:
        for v in (b, x, bf, xf, odd, short, short32, lv, short_lv):
            v.free()
        G.free()
    assert C.sizeof(C.c_double) == 8
