"""sh_ilu0 on the GPU: lu as float64 and float32 bit patterns, in place and not, level, the handle's figures, the footprint
and the figures and the plan of every call against tests/ilu0_ref.py's restatement (pinned against exact arithmetic and the
host gold by tests/test_ilu0_ref.py).  The cases are tests/ilu0_ref.py's CASES.

Every comparison is exact (==): the header fixes the order of every operation on a slot as a function of the pattern
alone and every slot has one owner; a NaN must stand where a NaN stands.  The shapes are the smallest at which a kernel
can still go wrong: rows on both sides of ILU0_LANE_WORK, rows k on both sides of a wave's stride (64) under a row of the
wave tier whose lower slots they write, a hub column, a level wider than a capped launch has lanes, more levels than the
analysis' first two batches hold, runs cut at ILU0_RUN, levels on both sides of `thin`."""
import numpy as np
import pytest

import guarded as GD
import ilu0_ref as R
from guarded import _not_halted   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine, EngineError
from sparseharness_amd.ilu0 import Ilu0Graph

pytestmark = pytest.mark.gpu

FIGURES = ("entries", "levels", "max_list", "max_width", "missing_diag", "first_missing", "work")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def factorise(eng, G, val, f32=1, thin=None, inplace=False):
    """-> (lu, (launches, runs, levels_in_runs), (zero_pivots, first_zero)) of one call on handle G."""
    val = np.ascontiguousarray(val, np.float32)
    nnz = len(val)
    host = np.zeros(max(nnz, 1), np.float32)
    host[:nnz] = val
    vv = eng.vector(host.view(np.uint32))
    lv = vv if inplace else eng.vector(np.full((1 if f32 else 2) * max(nnz, 1), 0x7FC00123, np.uint32))
    try:
        launches, runs, in_runs, zero, first, _ = GD.call(eng.ilu0, G, vv, lv, f32, thin)
        lu = lv.download(np.uint32, (1 if f32 else 2) * nnz).view(np.float32 if f32 else np.float64)
        if not inplace:   # val is read only
            assert np.array_equal(vv.download(np.uint32, host.size), host.view(np.uint32))
        return lu, (launches, runs, in_runs), (zero, first)
    finally:
        vv.free()
        if not inplace:
            lv.free()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not R.same_bits(got, want):
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        bad = np.nonzero((got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want)))[0]
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist()))


def the_plan(name, thin=None):
    w = R.want(name)
    return R.plan(w["lstart"], thin, w["entries"], len(R.case(name)[2]))


# ---- 1. against the restatement: float64, float32, in place, the figures, the footprint, the levels, the default plan
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_equals_the_restatement_bit_for_bit(eng, name):
    mat, w, w64 = R.case(name), R.want(name, 1), R.want(name, 0)
    n, nnz = mat[0], len(mat[2])
    G = eng.ilu0_graph(mat[1], mat[2])
    lv = eng.vector(np.full(max(n, 1), 7, np.int32))
    try:
        assert isinstance(G, Ilu0Graph)
        assert {k: getattr(G, k) for k in FIGURES} == {k: w[k] for k in FIGURES}, name
        assert G.edges == w["entries"] and G.footprint == R.header_footprint(n, nnz, w["entries"], w["levels"])
        G.level(lv)
        assert np.array_equal(lv.download(np.int32, n), w["level"]), name
        lu, plan, zero = factorise(eng, G, mat[3], f32=0)
        same(lu, w64["lu"], name + " f64")
        assert plan == the_plan(name) and zero == (w["zero_pivots"], w["first_zero"]), name
        for inplace in (False, True):
            lu, plan, zero = factorise(eng, G, mat[3], f32=1, inplace=inplace)
            same(lu, w["lu"], name + " f32" + " in place" * inplace)
            assert plan == the_plan(name) and zero == (w["zero_pivots"], w["first_zero"]), name
        if name in R.NOTHING:
            assert plan == (0, 0, 0)   # nothing launched
    finally:
        lv.free()
        G.free()


# ---- 2. the plan and thin: lu does not depend on it
@pytest.mark.parametrize("name", ("widths64", "widths256", "path-runs", "tiers"))
def test_the_plan_is_the_restated_one_and_lu_does_not_depend_on_thin(eng, name):
    mat, w = R.case(name), R.want(name, 0)
    G = eng.ilu0_graph(mat[1], mat[2])
    try:
        for thin in (0, 1, 64, None, R.THIN_MAX):
            lu, plan, _ = factorise(eng, G, mat[3], f32=0, thin=thin)
            same(lu, w["lu"], (name, thin))
            assert plan == the_plan(name, thin), (name, thin)
    finally:
        G.free()
    if name == "path-runs":   # runs are cut at the cap: 1024 + 1024 + 3 levels, between ilu0_load and ilu0_store
        assert the_plan(name) == (5, 3, 2 * R.RUN + 3) and the_plan(name, 0) == (2 * R.RUN + 5, 0, 0)
    if name == "widths64":
        assert the_plan(name, 64) == (6, 2, 3)


# ---- 3. handles: one pattern, new values
def test_refactorisation_on_one_handle_interleaved_with_a_second_handle(eng):
    a, b = R.case("drawn40"), R.case("grid12")
    rng = np.random.default_rng(12)
    vals_a = [a[3], (a[3] * rng.uniform(0.5, 1.5, len(a[3]))).astype(np.float32)]
    vals_b = [b[3], (b[3] * rng.uniform(0.9, 1.1, len(b[3]))).astype(np.float32)]
    GA, GB = eng.ilu0_graph(a[1], a[2]), eng.ilu0_graph(b[1], b[2])
    try:
        for k in (0, 1, 0, 1, 1):
            la, _, _ = factorise(eng, GA, vals_a[k], f32=0)
            lb, _, _ = factorise(eng, GB, vals_b[k], f32=0)
            for mat, vals, got in ((a, vals_a[k], la), (b, vals_b[k], lb)):
                same(got, R.factor((mat[0], mat[1], mat[2], vals), 0)["lu"], ("values", k))
                fresh = eng.ilu0_graph(mat[1], mat[2])
                try:
                    same(got, factorise(eng, fresh, vals, f32=0)[0], ("a fresh handle", k))
                finally:
                    fresh.free()
    finally:
        GA.free()
        GB.free()


@pytest.mark.parametrize("name", ("grid12", "tiers", "dirt", "path-runs"))
def test_level_is_the_triangular_solve_handle_s_level(eng, name):
    mat = R.case(name)
    n = mat[0]
    G, TG = eng.ilu0_graph(mat[1], mat[2]), eng.trsv_graph(mat[1], mat[2], mat[3], 0, 1)
    a, b = eng.vector(np.full(n, 7, np.int32)), eng.vector(np.full(n, 9, np.int32))
    try:
        G.level(a)
        TG.level(b)
        assert np.array_equal(a.download(np.int32, n), b.download(np.int32, n))
        assert G.levels == TG.levels and G.max_width == TG.max_width
    finally:
        for v in (a, b, G, TG):
            v.free()


# ---- 4. end to end: the float32 lu is L and U for sh_trsv
@pytest.mark.parametrize("name", R.EXACT)
def test_the_downloaded_factor_solves_exactly_through_two_trsv_handles(eng, name):
    mat, L0, U0 = R.exact_case(name[len("exact-"):])
    n = mat[0]
    G = eng.ilu0_graph(mat[1], mat[2])
    try:
        lu, _, zero = factorise(eng, G, mat[3])
    finally:
        G.free()
    assert zero == (0, -1)
    x0 = np.random.default_rng(13).integers(-3, 4, n).astype(np.float64)
    rhs = (L0 @ U0) @ x0   # small integers: exact
    GL, GU = eng.trsv_graph(mat[1], mat[2], lu, 0, 1), eng.trsv_graph(mat[1], mat[2], lu, 1, 0)
    bv, yv, xv = (eng.vector(v.view(np.uint32)) for v in (rhs, np.zeros(n), np.zeros(n)))
    try:
        GD.call(eng.trsv, GL, bv, yv)
        GD.call(eng.trsv, GU, yv, xv)
        assert np.array_equal(yv.download(np.uint32, 2 * n).view(np.float64), U0 @ x0)
        assert np.array_equal(xv.download(np.uint32, 2 * n).view(np.float64), x0)   # x == x0 exactly
    finally:
        for v in (bv, yv, xv, GL, GU):
            v.free()


# ---- 5. the buffers and the refusals
def test_only_the_stated_elements_change_and_argument_errors_leave_the_buffers_alone(eng):
    mat, w, w64 = R.case("drawn40"), R.want("drawn40", 1), R.want("drawn40", 0)
    n, nnz = mat[0], len(mat[2])
    lib = abi.load()
    dev = GD.Dev(lib, eng.h)
    G = eng.ilu0_graph(mat[1], mat[2])
    spare = 6
    fill = np.full(2 * nnz + spare, 7, np.int32)
    v32 = np.full(nnz + spare, 7, np.int32)
    v32[:nnz] = mat[3].view(np.int32)
    val, lu, lf = dev.guarded(v32, offset=2), dev.guarded(fill, offset=4), dev.guarded(fill[:nnz + spare], offset=3)
    bystander, inplace = dev.guarded(fill, offset=2), dev.guarded(v32, offset=5)
    odd, short, short32 = dev.guarded(fill, offset=1), dev.guarded(fill[:2 * nnz - 1], offset=0), dev.guarded(fill[:nnz - 1], offset=0)
    lv, short_lv = dev.guarded(fill[:n + spare], offset=1), dev.guarded(fill[:n - 1], offset=0)
    try:
        GD.call(eng.ilu0, G, val, lu, 0)
        got = lu.read("lu")
        assert (got[2 * nnz:] == 7).all() and np.array_equal(got[:2 * nnz], w64["lu"].view(np.uint32))
        GD.call(eng.ilu0, G, val, lf, 1)
        got = lf.read("lu f32")
        assert (got[nnz:] == 7).all() and np.array_equal(got[:nnz], w["lu"].view(np.uint32))
        GD.call(eng.ilu0, G, inplace, inplace, 1)
        got = inplace.read("in place")
        assert (got[nnz:] == 7).all() and np.array_equal(got[:nnz], w["lu"].view(np.uint32))
        assert np.array_equal(val.read("val"), v32.view(np.uint32))   # val is read only when lu is another vector
        assert (bystander.read("a vector no call was given") == 7).all()
        G.level(lv)
        got = lv.read("level")
        assert (got[n:] == 7).all() and np.array_equal(got[:n].view(np.int32), w["level"])
        dev.ok(lib.sh_vec_upload(eng.h, lu.v, GD.vp(fill), len(fill)))
        overlap = eng.wrap(lib.sh_vec_device_ptr(val.v) + 8, 2 * nnz)
        overlap32 = eng.wrap(lib.sh_vec_device_ptr(val.v) + 4, nnz)
        bad_calls = (
            (dict(f32=2), abi.SH_EINVAL, "f32"),
            (dict(thin=R.THIN_MAX + 1), abi.SH_EINVAL, "thin"),
            (dict(val=short32), abi.SH_ESHAPE, "val holds"),
            (dict(lu=short), abi.SH_ESHAPE, "lu holds"),
            (dict(lu=short32, f32=1), abi.SH_ESHAPE, "lu holds"),
            (dict(lu=odd), abi.SH_EINVAL, "aligned"),
            (dict(lu=overlap), abi.SH_EINVAL, "overlap"),
            (dict(lu=overlap32, f32=1), abi.SH_EINVAL, "overlap"),
            (dict(val=lu), abi.SH_EINVAL, "overlap"),   # the same vector is for float32 only
        )
        for change, code, word in bad_calls:
            args = dict(val=val, lu=lu, f32=0, thin=None)
            args.update(change)
            with pytest.raises(EngineError) as err:
                eng.ilu0(G, **args)
            assert err.value.code == code and word in str(err.value) and "sh_ilu0" in str(err.value), (change, str(err.value))
        with pytest.raises(EngineError) as err:
            G.level(short_lv)
        assert err.value.code == abi.SH_ESHAPE and "level" in str(err.value)
        overlap.free()
        overlap32.free()
        assert (lu.read("after the refused calls") == 7).all() and (odd.read("odd") == 7).all()
        assert np.array_equal(val.read("val after the refused calls"), v32.view(np.uint32))
        # an odd float32 offset is fine: only a float64 lu must be 8-byte aligned
        GD.call(eng.ilu0, G, val, lf, 1, 0)
        assert np.array_equal(lf.read("lu f32 again")[:nnz], w["lu"].view(np.uint32))
    finally:
        for v in (val, lu, lf, bystander, inplace, odd, short, short32, lv, short_lv):
            v.free()
        G.free()
