"""Every run-ahead loop walked across its batch seams on the device, through the C ABI with ctypes: sh_iterate,
sh_iterate_multi, sh_bits_iterate, sh_iterate_frontier (batches of 8 launches) and, through run_batches, sh_bfs_levels,
sh_core, sh_truss, sh_sssp, sh_scc and sh_wcc (batches of 8, 16, 32, 32 steps).  The inputs and their references are
those of tests/seam_shapes.py; tests/test_seams_cpu.py proves that they end on launch 7, 8, 9, ... as claimed.

Exact tier: the confirming launch on every value of the seam set, then the caps count - 1, count, count + 1 on the same
upload or handle, then one more uncapped run; vectors, counts and records == the references (O.iterate, oracle_bfs,
core_ref.peel, truss_ref.peel), never anything read from the device.  Invariant tier (sh_sssp, sh_scc, sh_wcc, whose
step counts are not modelled): what every correct run satisfies, at every cap of the seam set.

Every per-launch output array is 4 entries longer than its documented capacity and prefilled with a pattern: entries
[0, count) must be written, everything behind must still hold the pattern (sh_bits_iterate's newly_set is zeroed in
full by contract: zeros from `launches` to its capacity, the pattern behind).  The comb's hub row is above the
long-row threshold of the CSR-stream plan and heavy for the tiled plan, asserted from describe(), so the gated fix-up
kernels of every family run in every launch.  All data is integer-valued; every comparison is == on the bits."""
import ctypes as C
import re

import numpy as np
import pytest

import seam_shapes as S
import test_bfs_levels_gpu as BL
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine

pytestmark = pytest.mark.gpu

PAT = {np.int32: 0x5A5A5A5A, np.uint32: 0x5A5A5A5A, np.int64: 0x5A5A5A5A5A5A5A5A, np.uint64: 0x5A5A5A5A5A5A5A5A}
CT = {np.int32: C.c_int32, np.uint32: C.c_uint32, np.int64: C.c_int64, np.uint64: C.c_uint64}
GUARD = 4
UPLOADS = {"stream": dict(plan=1), "tiled": dict(plan=2), "bits": dict(or_and_bits=2)}
INF = float("inf")
_halt = []   # why the module's GPU work ended early (a HIP call that failed)


def uploads_of(sr):
    return ("stream", "tiled", "bits") if sr == S.OA else ("stream", "tiled")


class Out:
    """A per-launch output array of `cap` documented entries, GUARD more behind them, all prefilled with a pattern."""

    def __init__(self, cap, dtype, width=1):
        self.cap, self.dtype, self.width = cap, dtype, width
        self.a = np.full((cap + GUARD) * width, PAT[dtype], dtype)

    @property
    def p(self):
        return self.a.ctypes.data_as(C.POINTER(CT[self.dtype]))

    def taken(self, count, what, written=True):
        """-> entries [0, count); asserts that the rest still holds the pattern (and, `written`, that they do not)."""
        count *= self.width
        assert 0 <= count <= self.cap * self.width, (what, count, self.cap)
        rest = self.a[count:]
        bad = np.nonzero(rest != PAT[self.dtype])[0]
        assert len(bad) == 0, f"{what}: written past its count {count // self.width}: entries {(count + bad[:6]).tolist()}"
        if written:
            assert (self.a[:count] != PAT[self.dtype]).all(), f"{what}: an entry below the count {count // self.width} was not written"
        return self.a[:count].copy()


def p_scalar(sr, v):
    return np.array([v], np.int32 if sr in (S.OA, S.MM) else np.float32)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Ctx:
    def __init__(self):
        self.eng, self.lib = Engine(0), abi.load()
        self.mats, self.fronts = {}, {}

    def ok(self, rc):
        msg = (self.lib.sh_last_error(self.eng.h) or b"").decode() if rc else ""
        if rc == abi.SH_EHIP:
            _halt.append(msg)
        assert rc == abi.SH_OK, (rc, msg)

    def mat(self, sr, L, up):
        """The matrix of seam_shapes.iterate_case(sr, L) under an upload, made once; its fix-up rows asserted."""
        c = S.iterate_case(sr, L)
        key = (sr, c["n_path"], up)
        if key not in self.mats:
            A = self.eng.upload_csr(c["N"], c["N"], c["rp"], c["ci"], c["va"], **UPLOADS[up])
            d = A.describe()
            if up == "stream":
                assert d.startswith("stream") and int(re.search(r"long_rows=(\d+)", d).group(1)) > 0, d
            elif up == "tiled":
                assert d.startswith("tiled") and int(re.search(r"heavy_rows=(\d+)", d).group(1)) > 0, d
            else:
                assert "or_and=bits(" in d and "only" in d, d
            self.mats[key] = A
        return self.mats[key]

    def front(self, sr, L, up):
        c = S.iterate_case(sr, L)
        key = (sr, c["n_path"], up)
        if key not in self.fronts:
            self.fronts[key] = self.eng.frontier(self.mat(sr, L, up), c["rp"], c["ci"], c["va"])
        return self.fronts[key]

    def close(self):
        for h in list(self.fronts.values()) + list(self.mats.values()):
            h.free()
        self.eng.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _not_halted(ctx):
    """After a failed HIP call nothing more of this module is started on the device."""
    if not _halt and ctx.lib.sh_engine_synchronize(ctx.eng.h) != abi.SH_OK:
        _halt.append("sh_engine_synchronize failed: " + (ctx.lib.sh_last_error(ctx.eng.h) or b"").decode())
    if _halt:
        pytest.fail("the module's GPU work ended at: " + _halt[0])


def same_bits(got, want, what):
    bad = np.nonzero(S.bits_of(got) != S.bits_of(want))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(want)} words differ, first at {bad[:6].tolist()}: got "
                           f"{S.bits_of(got)[bad[:6]].tolist()} want {S.bits_of(want)[bad[:6]].tolist()}")


# ------------------------------------------------------------------ sh_iterate
def call_iterate(ctx, sr, A, c, cap, what):
    dt = np.int32 if sr in (S.OA, S.MM) else np.float32
    eng = ctx.eng
    xv, yv, sc = eng.vector(c["x0"]), eng.vector(c["x0"]), eng.alloc(c["N"]).fill(0x6B6B6B6B, np.uint32)
    iters, conv, total = C.c_int32(-1), C.c_int32(-1), C.c_uint64(0)
    per = Out(cap, np.uint64)
    a, b = p_scalar(sr, c["alpha"]), p_scalar(sr, c["beta"])
    try:
        ctx.ok(ctx.lib.sh_iterate(eng.h, sr, A.h, xv.h, yv.h, sc.h, vp(a), vp(b), S.DELTA, cap, None, C.byref(iters),
                                  C.byref(conv), per.p, C.byref(total)))
        got = xv.download(dt)
    finally:
        for v in (xv, yv, sc):
            v.free()
    ns = per.taken(iters.value, what + " ns_per_iter")
    assert total.value == int(ns.sum()), what
    return got, iters.value, bool(conv.value)


def runs_of(L):
    """(cap, label) of the runs on one upload, in order: uncapped, the three caps, uncapped again."""
    return [(S.UNCAPPED, "uncapped")] + [(c, f"cap {c}") for c in S.caps_for(L)] + [(S.UNCAPPED, "uncapped, after the caps")]


@pytest.mark.parametrize("L", S.S8)
@pytest.mark.parametrize("sr", (S.PT, S.MP, S.OA, S.MM), ids=S.SR_NAME.get)
def test_iterate_confirms_on_every_launch_around_a_seam(ctx, sr, L):
    c = S.iterate_case(sr, L)
    for up in uploads_of(sr):
        A = ctx.mat(sr, L, up)
        for cap, label in runs_of(L):
            what = f"sh_iterate {S.SR_NAME[sr]} {up} L={L} {label}"
            want, w_it, w_conv = S.iterate_ref(sr, L, cap)
            got, it, conv = call_iterate(ctx, sr, A, c, cap, what)
            assert (it, conv) == (w_it, w_conv) == (min(cap, L), cap >= L), (what, it, conv)
            same_bits(got, want, what)


# ------------------------------------------------------------------ sh_iterate_multi
def call_multi(ctx, sr, A, X0, width, cap, what):
    dt = X0.dtype
    eng, n = ctx.eng, X0.shape[0]
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0x6B6B6B6B, np.uint32)
    launches, total = C.c_int32(-1), C.c_uint64(0)
    iters, conv, per = Out(width, np.int32), Out(width, np.int32), Out(cap, np.uint64)
    a, b = p_scalar(sr, S.SCALARS[sr][0]), p_scalar(sr, S.SCALARS[sr][1])
    try:
        ctx.ok(ctx.lib.sh_iterate_multi(eng.h, sr, A.h, width, xv.h, yv.h, sc.h, vp(a), vp(b), S.DELTA, cap, C.byref(launches),
                                        iters.p, conv.p, per.p, C.byref(total)))
        got = xv.download(dt, shape=(n, width))
    finally:
        for v in (xv, yv, sc):
            v.free()
    ns = per.taken(launches.value, what + " ns_per_launch")
    assert total.value == int(ns.sum()), what
    return got, launches.value, iters.taken(width, what + " iters").tolist(), conv.taken(width, what + " converged").tolist()


def multi_runs(counts):
    return [(S.UNCAPPED, "uncapped")] + [(c, f"cap {c}") for c in S.multi_caps(counts)] + [(S.UNCAPPED, "uncapped, after the caps")]


def check_multi(ctx, sr, counts):
    width = len(counts)
    A = ctx.mat(sr, counts[0], "stream")
    N = S.iterate_case(sr, counts[0])["N"]
    X0 = np.ascontiguousarray(np.stack([S.iterate_case(sr, L)["x0"] for L in counts], axis=1))
    assert X0.shape == (N, width)
    for cap, label in multi_runs(counts):
        what = f"sh_iterate_multi {S.SR_NAME[sr]} width {width} counts {counts[:8]} {label}"
        refs = [S.source_ref(sr, L, cap) for L in counts]
        got, launches, iters, conv = call_multi(ctx, sr, A, X0, width, cap, what)
        assert iters == [r[1] for r in refs] == [min(L, cap) for L in counts], (what, iters)
        assert conv == [int(r[2]) for r in refs], (what, conv)
        assert launches == max(iters), (what, launches)
        for j in range(width):
            same_bits(got[:, j], refs[j][0], f"{what} column {j} (count {counts[j]})")


@pytest.mark.parametrize("counts", S.COUNTS4 + (S.COUNTS32,), ids=lambda c: f"w{len(c)}-{'-'.join(map(str, c[:4]))}")
@pytest.mark.parametrize("sr", (S.OA, S.MP), ids=S.SR_NAME.get)
def test_iterate_multi_freezes_columns_in_three_batches(ctx, sr, counts):
    check_multi(ctx, sr, counts)


# ------------------------------------------------------------------ sh_bits_iterate
def call_bits(ctx, A, P0, words, cap, what):
    eng, n = ctx.eng, P0.shape[0]
    n_src = 32 * words
    xv, yv, sc = eng.vector(P0), eng.vector(P0), eng.alloc(n * words).fill(0x6B6B6B6B, np.uint32)
    launches, total = C.c_int32(-1), C.c_uint64(0)
    iters, conv, per = Out(n_src, np.int32), Out(n_src, np.int32), Out(cap, np.uint64)
    newly = Out(cap, np.uint32, width=n_src)
    a, b = p_scalar(S.OA, 1), p_scalar(S.OA, 1)
    try:
        ctx.ok(ctx.lib.sh_bits_iterate(eng.h, A.h, words, xv.h, yv.h, sc.h, vp(a), vp(b), cap, C.byref(launches), iters.p, conv.p,
                                       newly.p, per.p, C.byref(total)))
        got = xv.download(np.uint32, shape=(n, words))
    finally:
        for v in (xv, yv, sc):
            v.free()
    ns = per.taken(launches.value, what + " ns_per_launch")
    assert total.value == int(ns.sum()), what
    counted = newly.taken(cap, what + " newly_set", written=False).reshape(cap, n_src)   # zeroed in full, by contract
    assert (counted[launches.value:] == 0).all(), f"{what}: newly_set is not zero from launch {launches.value} on"
    return (got, launches.value, iters.taken(n_src, what + " iters").tolist(), conv.taken(n_src, what + " converged").tolist(),
            counted[:launches.value])


@pytest.mark.parametrize("words", (1, 8))
def test_bits_iterate_freezes_sources_in_three_batches(ctx, words):
    n_src = 32 * words
    counts = S.counts_of_sources(n_src)
    A = ctx.mat(S.OA, 1, "stream")
    N = S.iterate_case(S.OA, 1)["N"]
    P0 = np.zeros((N, words), np.uint32)
    for s, L in enumerate(counts):
        P0[S.source_for(S.OA, L), s // 32] |= np.uint32(1) << np.uint32(s % 32)
    for cap, label in multi_runs(counts):
        what = f"sh_bits_iterate words {words} {label}"
        refs = {L: S.source_ref(S.OA, L, cap) for L in set(counts)}
        got, launches, iters, conv, newly = call_bits(ctx, A, P0, words, cap, what)
        assert iters == [refs[L][1] for L in counts] == [min(L, cap) for L in counts], (what, iters[:32])
        assert conv == [int(refs[L][2]) for L in counts], (what, conv[:32])
        assert launches == max(iters), (what, launches)
        want = np.zeros((N, words), np.uint32)
        levels = np.zeros((launches, n_src), np.uint32)
        for s, L in enumerate(counts):
            want[:, s // 32] |= (refs[L][0] != 0).astype(np.uint32) << np.uint32(s % 32)
            sizes = S.level_sizes(L, iters[s])
            levels[:len(sizes), s] = sizes
        same_bits(got.ravel(), want.ravel(), what)
        assert np.array_equal(newly, levels), (what, np.argwhere(newly != levels)[:6].tolist())


# ------------------------------------------------------------------ sh_iterate_frontier
def call_frontier(ctx, sr, A, F, c, cap, share, what):
    dt = np.int32 if sr in (S.OA, S.MM) else np.float32
    eng = ctx.eng
    xv, yv, sc = eng.vector(c["x0"]), eng.vector(c["x0"]), eng.alloc(c["N"]).fill(0x6B6B6B6B, np.uint32)
    iters, conv, total = C.c_int32(-1), C.c_int32(-1), C.c_uint64(0)
    modes, changed, active, per = Out(cap, np.int32), Out(cap, np.int64), Out(cap, np.int64), Out(cap, np.uint64)
    a, b = p_scalar(sr, c["alpha"]), p_scalar(sr, c["beta"])
    try:
        ctx.ok(ctx.lib.sh_iterate_frontier(eng.h, sr, A.h, F.h, xv.h, yv.h, sc.h, vp(a), vp(b), S.DELTA, cap, share, C.byref(iters),
                                           C.byref(conv), modes.p, changed.p, active.p, per.p, C.byref(total)))
        got = xv.download(dt)
    finally:
        for v in (xv, yv, sc):
            v.free()
    n = iters.value
    ns = per.taken(n, what + " ns_per_iter")
    assert total.value == int(ns.sum()), what
    return (got, n, bool(conv.value), modes.taken(n, what + " mode_per_iter").tolist(),
            changed.taken(n, what + " changed_per_iter").tolist(), active.taken(n, what + " active_per_iter").tolist())


@pytest.mark.parametrize("L", S.S8)
@pytest.mark.parametrize("sr", (S.OA, S.MP), ids=S.SR_NAME.get)
def test_iterate_frontier_with_its_seams_where_the_mode_puts_them(ctx, sr, L):
    """dense_share 0: no launch is sparse and the seams lie at 8, 16, 24.  dense_share 1 and the default: every launch
    from 2 on is sparse (one changed row, one transposed entry), the first batch is cut behind launch 1 and the seams
    lie at 2, 10, 18, 26."""
    c = S.iterate_case(sr, L)
    for up in uploads_of(sr):
        A, F = ctx.mat(sr, L, up), ctx.front(sr, L, up)
        for share, rule in ((0.0, 0.0), (1.0, 1.0), (-1.0, 0.02)):
            for cap, label in runs_of(L):
                what = f"sh_iterate_frontier {S.SR_NAME[sr]} {up} dense_share {share} L={L} {label}"
                want, w_it, w_conv = S.iterate_ref(sr, L, cap)
                got, it, conv, modes, changed, active = call_frontier(ctx, sr, A, F, c, cap, share, what)
                assert (it, conv) == (w_it, w_conv) == (min(cap, L), cap >= L), (what, it, conv)
                same_bits(got, want, what)
                assert modes == S.frontier_modes(sr, L, it, rule), (what, modes)
                assert changed == S.frontier_changed(sr, L, it), (what, changed)
                assert all(a == c["N"] for a, m in zip(active, modes) if m == 0), (what, active)
                assert all(0 <= a <= c["N"] for a in active), (what, active)


# ------------------------------------------------------------------ sh_bfs_levels
def call_bfs(ctx, G, x0, cap, shares, steps, what):
    eng, n = ctx.eng, len(x0)
    xv, lv, pv = eng.vector(x0), eng.alloc(n).fill(7, np.int32), eng.alloc(n).fill(7, np.int32)
    depth, reached, complete, total = C.c_int32(-1), C.c_int64(-1), C.c_int32(-1), C.c_uint64(0)
    modes, sizes, edges, per = Out(cap, np.int32), Out(cap + 1, np.int64), Out(cap, np.int64), Out(cap, np.uint64)
    try:
        ctx.ok(ctx.lib.sh_bfs_levels(eng.h, G.h, xv.h, lv.h, pv.h, cap, shares[0], shares[1], C.byref(depth), C.byref(reached),
                                     C.byref(complete), modes.p, sizes.p, edges.p, per.p, C.byref(total)))
        level, parent = lv.download(np.int32), pv.download(np.int32)
    finally:
        for v in (xv, lv, pv):
            v.free()
    res = (depth.value, reached.value, bool(complete.value), modes.taken(steps, what + " mode_per_level"),
           sizes.taken(steps + 1, what + " size_per_level"), edges.taken(steps, what + " edges_per_level"),
           per.taken(steps, what + " ns_per_level"), total.value)
    return level, parent, res


@pytest.mark.parametrize("L", S.S32)
def test_bfs_levels_ends_on_every_step_around_a_seam(ctx, L):
    n, rp, ci, va, x0 = S.bfs_path(L)
    G = ctx.eng.bfs_graph(rp, ci, va)
    try:
        for shares in (BL.TOP_DOWN, BL.BOTTOM_UP, BL.DEFAULT):
            for cap in S.round_caps(L) + [S.UNCAPPED]:
                what = f"sh_bfs_levels path of {L} shares {shares} max_levels {cap}"
                b = S.bfs_ref(L, cap)
                assert (b.steps, b.complete) == (min(cap, L), cap >= L)
                level, parent, res = call_bfs(ctx, G, x0, cap, shares, b.steps, what)
                BL.check(b, level, parent, res, shares, what)
    finally:
        G.free()


# ------------------------------------------------------------------ sh_core and sh_truss
def call_core(ctx, G, n, cap, what):
    eng = ctx.eng
    cv, dv = eng.alloc(n).fill(7, np.int32), eng.alloc(n).fill(7, np.int32)
    degeneracy, levels, rounds, complete, total = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_uint64(0)
    ks, sizes, chased, edges, per = (Out(cap, np.int32), Out(cap, np.int64), Out(cap, np.int64), Out(cap, np.int64),
                                     Out(cap, np.uint64))
    try:
        ctx.ok(ctx.lib.sh_core(eng.h, G.h, cv.h, dv.h, 0, cap, C.byref(degeneracy), C.byref(levels), C.byref(rounds),
                               C.byref(complete), ks.p, sizes.p, chased.p, edges.p, per.p, C.byref(total)))
        core, deg = cv.download(np.int32), dv.download(np.int32)
    finally:
        cv.free()
        dv.free()
    r = rounds.value
    ns = per.taken(r, what + " ns_per_round")
    assert total.value >= int(ns.sum()), what
    return dict(core=core, deg=deg, degeneracy=degeneracy.value, levels=levels.value, rounds=r, complete=bool(complete.value),
                k=ks.taken(r, what + " k_per_round"), size=sizes.taken(r, what + " size_per_round"),
                chased=chased.taken(r, what + " chased_per_round"), edges=edges.taken(r, what + " edges_per_round"))


@pytest.mark.parametrize("R", S.S32)
def test_core_ends_on_every_round_around_a_seam(ctx, R):
    n, rp, ci, va = S.core_path(R)
    G = ctx.eng.core_graph(rp, ci, va)
    try:
        for cap in S.round_caps(R) + [n + 1]:
            what = f"sh_core path of {n} max_rounds {cap}"
            w = S.core_peel(R, cap)
            got = call_core(ctx, G, n, cap, what)
            assert (got["rounds"], got["complete"]) == (w["rounds"], w["complete"]) == (min(cap, R), cap >= R), (what, got["rounds"])
            for f in ("core", "deg", "k", "size", "edges"):
                assert np.array_equal(got[f], w[f]), (what, f, got[f][:8], w[f][:8])
            assert (got["chased"] == 0).all(), what
            if w["complete"]:
                assert (got["degeneracy"], got["levels"]) == (w["degeneracy"], w["levels"]), what
                assert int(got["size"].sum()) == n
    finally:
        G.free()


def call_truss(ctx, G, m, cap, what):
    eng = ctx.eng
    vecs = [eng.alloc(m).fill(7, np.int32) for _ in range(4)]
    max_truss, levels, rounds, complete = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    triangles, total = C.c_uint64(0), C.c_uint64(0)
    ks, sizes, walked, per = Out(cap, np.int32), Out(cap, np.int64), Out(cap, np.int64), Out(cap, np.uint64)
    try:
        ctx.ok(ctx.lib.sh_truss(eng.h, G.h, *(v.h for v in vecs), cap, C.byref(max_truss), C.byref(levels), C.byref(rounds),
                                C.byref(complete), C.byref(triangles), ks.p, sizes.p, walked.p, per.p, C.byref(total)))
        truss, support, edge_u, edge_v = (v.download(np.int32) for v in vecs)
    finally:
        for v in vecs:
            v.free()
    r = rounds.value
    ns = per.taken(r, what + " ns_per_round")
    assert total.value >= int(ns.sum()), what
    return dict(truss=truss, support=support, edge_u=edge_u, edge_v=edge_v, max_truss=max_truss.value, levels=levels.value,
                rounds=r, complete=bool(complete.value), triangles=triangles.value, k=ks.taken(r, what + " k_per_round"),
                size=sizes.taken(r, what + " size_per_round"), walked=walked.taken(r, what + " walked_per_round"))


@pytest.mark.parametrize("R", S.S32_TRUSS)
def test_truss_ends_on_every_round_around_a_seam(ctx, R):
    n, rp, ci, va = S.truss_cliques(R)
    G = ctx.eng.truss_graph(rp, ci, va)
    try:
        m = G.edges
        for cap in S.round_caps(R) + [m + 1]:
            what = f"sh_truss K3..K{R + 2} max_rounds {cap}"
            # (a cap of R or more never stops truss_ref.peel: its answer is the uncapped one, which test_seams_cpu.py pins,
            # and one 2 s reference run per case is spared)
            w = S.truss_peel(R, cap if cap < R else None)
            assert m == w["M"]
            got = call_truss(ctx, G, m, cap, what)
            assert (got["rounds"], got["complete"]) == (w["rounds"], w["complete"]) == (min(cap, R), cap >= R), (what, got["rounds"])
            for f in ("truss", "support", "edge_u", "edge_v", "k", "size", "walked"):
                assert np.array_equal(got[f], w[f]), (what, f, got[f][:8], w[f][:8])
            assert got["triangles"] == w["triangles"], what
            if w["complete"]:
                assert (got["max_truss"], got["levels"]) == (w["max_truss"], w["levels"]), what
                assert int(got["size"].sum()) == m
    finally:
        G.free()


# ------------------------------------------------------------------ the invariant tier: sh_sssp, sh_scc, sh_wcc
def call_sssp(ctx, G, x0, delta, cap, what):
    eng, n = ctx.eng, len(x0)
    xv, dv, pv = eng.vector(x0), eng.alloc(n).fill(7.0), eng.alloc(n).fill(7, np.int32)
    rounds, buckets, reached, complete = C.c_int32(-1), C.c_int32(-1), C.c_int64(-1), C.c_int32(-1)
    relaxed, total = C.c_int64(-1), C.c_uint64(0)
    sizes, edges, per = Out(cap, np.int64), Out(cap, np.int64), Out(cap, np.uint64)
    try:
        ctx.ok(ctx.lib.sh_sssp(eng.h, G.h, xv.h, dv.h, pv.h, delta, cap, C.byref(rounds), C.byref(buckets), C.byref(reached),
                               C.byref(complete), C.byref(relaxed), sizes.p, edges.p, per.p, C.byref(total)))
        dist, pred = dv.download(np.float32), pv.download(np.int32)
    finally:
        for v in (xv, dv, pv):
            v.free()
    r = rounds.value
    ns = per.taken(r, what + " ns_per_round")
    sizes.taken(r, what + " size_per_round")
    edges.taken(r, what + " edges_per_round")
    assert total.value >= int(ns.sum()), what
    return dist, pred, r, bool(complete.value), reached.value


@pytest.mark.parametrize("delta", (1.0, INF), ids=("delta-1", "one-bucket"))
def test_sssp_cut_at_every_seam(ctx, delta):
    n, rp, ci, va, x0 = S.sssp_path()
    w_dist, w_pred, w_reached = S.sssp_want()
    G = ctx.eng.sssp_graph(rp, ci, va)

    def complete_and_right(dist, pred, reached, what):
        same_bits(dist, w_dist, what + " dist")
        assert np.array_equal(pred, w_pred) and reached == w_reached, what

    try:
        what = f"sh_sssp path of {n} delta {delta}"
        dist, pred, rounds, complete, reached = call_sssp(ctx, G, x0, delta, S.UNCAPPED, what + " uncapped")
        assert rounds >= 90, f"{what}: the input is too short for the caps, {rounds} rounds"   # (a check of the input)
        assert complete
        complete_and_right(dist, pred, reached, what + " uncapped")
        for cap in S.S32:
            dist, pred, rounds, complete, reached = call_sssp(ctx, G, x0, delta, cap, f"{what} cap {cap}")
            assert rounds <= cap and (complete or rounds == cap), (what, cap, rounds, complete)
            if complete:
                complete_and_right(dist, pred, reached, f"{what} cap {cap}")
            else:   # between the fixed point and the start, word for word (non-negative floats order as their bits)
                assert (S.bits_of(w_dist) <= S.bits_of(dist)).all() and (S.bits_of(dist) <= S.bits_of(x0)).all(), (what, cap)
        dist, pred, rounds, complete, reached = call_sssp(ctx, G, x0, delta, S.UNCAPPED, what + " uncapped, after the caps")
        assert complete
        complete_and_right(dist, pred, reached, what + " uncapped, after the caps")
    finally:
        G.free()


def call_scc(ctx, G, n, cap, what):
    eng = ctx.eng
    cv = eng.alloc(n).fill(7, np.int32)
    components, settled, trimmed = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rounds, steps, complete, total = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_uint64(0)
    kinds, sizes, steps_per, edges, per = (Out(cap, np.int32), Out(cap, np.int64), Out(cap, np.int32), Out(cap, np.int64),
                                           Out(cap, np.uint64))
    try:
        ctx.ok(ctx.lib.sh_scc(eng.h, G.h, cv.h, 0, 0, cap, C.byref(components), C.byref(settled), C.byref(trimmed), C.byref(rounds),
                              C.byref(steps), C.byref(complete), kinds.p, sizes.p, steps_per.p, edges.p, per.p, C.byref(total)))
        comp = cv.download(np.int32)
    finally:
        cv.free()
    r = rounds.value
    assert 0 <= r <= steps.value, (what, r, steps.value)
    ns = per.taken(r, what + " ns_per_round")
    edges.taken(r, what + " edges_per_round")
    assert total.value >= int(ns.sum()), what
    return dict(comp=comp, components=components.value, settled=settled.value, rounds=r, steps=steps.value,
                complete=bool(complete.value), kinds=kinds.taken(r, what + " kind_per_round"),
                size=sizes.taken(r, what + " size_per_round"), steps_per=steps_per.taken(r, what + " steps_per_round"))


def test_scc_cut_at_every_seam(ctx):
    n, rp, ci, va = S.scc_path()
    ref = S.scc_want()
    G = ctx.eng.scc_graph(rp, ci, va)

    def complete_and_right(got, what):
        assert got["complete"] and np.array_equal(got["comp"], ref), what
        assert (got["components"], got["settled"]) == (n, n) and got["kinds"].tolist() == [2] * n, what
        assert got["size"].tolist() == [1] * n, what

    try:
        what = f"sh_scc path of {n} without trim and pivot"
        full = call_scc(ctx, G, n, 1 << 16, what + " uncapped")
        complete_and_right(full, what + " uncapped")
        # (a check of the input: every cap below cuts.  A colouring round is a seed sweep, a propagation sweep per hop and
        # the claim sweeps; the last vertex alone has been seen to take 3 steps, every other round more.)
        assert full["steps"] > max(S.S32) and (full["steps_per"] >= 3).all(), (what, full["steps"], full["steps_per"])
        for cap in S.S32:
            got = call_scc(ctx, G, n, cap, f"{what} cap {cap}")
            done = got["comp"] != -1
            assert got["steps"] <= cap and (got["complete"] or got["steps"] == cap), (what, cap, got["steps"])
            assert got["complete"] == bool(done.all()), (what, cap)
            assert np.array_equal(got["comp"][done], ref[done]), (what, cap)              # only final labels appear
            assert got["settled"] == int(done.sum()) == int(got["size"].sum()), (what, cap)
            assert got["components"] == int(np.count_nonzero(got["comp"] == np.arange(n))), (what, cap)
            assert int(got["steps_per"].sum()) <= got["steps"], (what, cap)
            if got["complete"]:
                complete_and_right(got, f"{what} cap {cap}")
        complete_and_right(call_scc(ctx, G, n, 1 << 16, what + " uncapped, after the caps"), what + " uncapped, after the caps")
    finally:
        G.free()


def call_wcc(ctx, G, n, sample, cap, what):
    eng = ctx.eng
    cv = eng.alloc(n).fill(7, np.int32)
    components, skipped = C.c_int64(-1), C.c_int64(-1)
    rounds, complete, total = C.c_int32(-1), C.c_int32(-1), C.c_uint64(0)
    kinds, hooks, jumps, edges, per = (Out(cap, np.int32), Out(cap, np.int64), Out(cap, np.int64), Out(cap, np.int64),
                                       Out(cap, np.uint64))
    try:
        ctx.ok(ctx.lib.sh_wcc(eng.h, G.h, cv.h, sample, cap, C.byref(components), C.byref(skipped), C.byref(rounds),
                              C.byref(complete), kinds.p, hooks.p, jumps.p, edges.p, per.p, C.byref(total)))
        comp = cv.download(np.int32)
    finally:
        cv.free()
    r = rounds.value
    ns = per.taken(r, what + " ns_per_round")
    for o, name in ((hooks, "hooks"), (jumps, "jumps"), (edges, "edges")):
        o.taken(r, f"{what} {name}_per_round")
    assert total.value >= int(ns.sum()), what
    return comp, components.value, r, bool(complete.value), kinds.taken(r, what + " kind_per_round").tolist()


@pytest.mark.parametrize("sample", S.WCC_SAMPLES)
def test_wcc_sampling_rounds_cross_the_seams(ctx, sample):
    n, rp, ci, va = S.wcc_grid()
    ref = S.wcc_want()
    G = ctx.eng.wcc_graph(rp, ci, va)

    def complete_and_right(comp, components, rounds, kinds, what):
        assert np.array_equal(comp, ref) and components == 1, what
        assert rounds > sample and kinds[:sample] == [0] * sample and set(kinds[sample:]) == {1}, (what, rounds, kinds)

    try:
        what = f"sh_wcc grid of {n} sample {sample}"
        comp, components, rounds, complete, kinds = call_wcc(ctx, G, n, sample, S.UNCAPPED, what + " uncapped")
        assert complete
        complete_and_right(comp, components, rounds, kinds, what + " uncapped")
        above = [c for c in S.S32 if c > sample + 1][:1]            # one cap that the run may or may not reach
        for cap in [c for c in S.S32 if c <= sample + 1] + above:
            comp, components, rounds, complete, kinds = call_wcc(ctx, G, n, sample, cap, f"{what} cap {cap}")
            assert rounds <= cap and (complete or rounds == cap), (what, cap, rounds, complete)
            assert kinds[:sample] == [0] * min(sample, rounds), (what, cap, kinds)
            if cap <= sample:
                assert not complete, (what, cap)
            if complete:
                complete_and_right(comp, components, rounds, kinds, f"{what} cap {cap}")
            else:   # a half-built forest is no partition
                assert (comp == -1).all() and components == 0, (what, cap)
        comp, components, rounds, complete, kinds = call_wcc(ctx, G, n, sample, S.UNCAPPED, what + " uncapped, after the caps")
        assert complete
        complete_and_right(comp, components, rounds, kinds, what + " uncapped, after the caps")
    finally:
        G.free()
