"""(or,and) and (max,min) on arbitrary int32 words, on the GPU, every path: sh_spmv under the five plan variants, both
builders and the bit-blocked layout; sh_spmm / sh_iterate_multi; sh_iterate / sh_iterate_frontier; the packed-bit entry
points; sh_bfs_graph_create / sh_bfs_levels; the device builders; the multi-GPU seam.

The words come from tests/int_ref.py: a third of them from its SPECIAL pool (INT_MIN = -0.0, INT_MAX, +-Inf, quiet and
signalling NaN patterns, subnormals, 2^24 + 1, the halves of a word), the rest uniform over all 2^32 words.  The reference is
int_ref.kernel / int_ref.iterate (numpy, from the definition; pinned against the C oracle in tests/test_int_ref.py, which
also shows that these inputs see a float-view compare, a compare by subtraction, a trip through float, a 16-bit truncation
and a padding 0).  Both semirings are exact and order-free: EVERY comparison here is == on uint32 views.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import graph_patterns as P
import int_ref as I
import test_bfs_levels_gpu as BL
from oracle import oracle as O
from sparseharness_amd.engine import Engine
from test_bits_gpu import column, one_hot, pack
from test_bits_gpu import ragged_csr as bits_ragged_csr
from test_builder_gpu import SHAPES as BUILDER_SHAPES
from test_builder_gpu import _p, compare, random_matrix, tools  # noqa: F401  (tools: the fixture of the tools library)
from test_multi_gpu import interleave, ragged_csr, run_spmm, run_spmv
from test_parity_gpu import clustered_matrix

pytestmark = pytest.mark.gpu

bits = I.bits
SEMIRINGS = [O.OR_AND_I32, O.MAX_MIN_I32]
SR_ID = {O.OR_AND_I32: "or_and", O.MAX_MIN_I32: "max_min"}.get
WIDTHS = [4, 8, 16, 32]
PLANS = ["stream", "tiled", "tiled-8bit", "tiled-raw", "tiled-nofold"]
TCOLS = 32760                      # columns of one x tile of the tiled plan


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(params=PLANS)
def plan(request, monkeypatch):
    """The plan variants of tests/test_parity_gpu.py's fixture; -> the variant's name."""
    monkeypatch.setenv("SH_PLAN", request.param.split("-")[0])
    monkeypatch.setenv("SH_VALCODE", {"raw": "off", "8bit": "8"}.get(request.param.split("-")[-1], "auto"))
    monkeypatch.setenv("SH_FOLD", "0" if request.param.endswith("nofold") else "1")
    return request.param


GENERATORS = I.generators(clustered_matrix)
# values=... of describe() per few-values input and plan variant (plan_common.h, decide_value_coding); the word sets hold a 0
CODING = {("few16", "tiled"): "dict4(16)", ("few16", "tiled-nofold"): "dict4(16)", ("few16", "tiled-8bit"): "dict8(16)",
          ("few255", "tiled"): "dict8(255)", ("few255", "tiled-nofold"): "dict8(255)", ("few255", "tiled-8bit"): "dict8(255)",
          ("few4000", "tiled"): "dict16(4000)", ("few4000", "tiled-nofold"): "dict16(4000)", ("few4000", "tiled-8bit"): "raw",
          ("few16", "tiled-raw"): "raw", ("few255", "tiled-raw"): "raw", ("few4000", "tiled-raw"): "raw"}


@functools.lru_cache(maxsize=None)
def data(name, sr):
    """An input set, with the reference of every epilogue computed once (want())."""
    if name == "all_negative":
        c = I.all_negative(data("ragged", sr))
    elif name == "dead_tiles":
        c = I.dead_tiles(data("wide", sr), TCOLS, live_tiles=(3, 40, 76))
    else:
        c = GENERATORS[name](sr)
    c = dict(c, name=name, want={})
    return c


def want(c, k):
    if k not in c["want"]:
        alpha, beta, with_y = I.EPILOGUES[c["sr"]][k]
        c["want"][k] = I.kernel(c["sr"], c["rp"], c["ci"], c["va"], c["x"], c["y"] if with_y else None, alpha, beta, c["cols"])
    return c["want"][k]


def assert_words(got, ref, what):
    bad = np.nonzero(bits(got) != bits(ref))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(ref)} words differ, first rows {bad[:6].tolist()}: "
                           f"got {[hex(v) for v in bits(got)[bad[:6]]]} want {[hex(v) for v in bits(ref)[bad[:6]]]}")


def spmv_all_epilogues(eng, c, A, what):
    """-> the outputs of every epilogue of c's semiring through device matrix A, each compared with the reference."""
    sr = c["sr"]
    xv, yv, out = eng.vector(c["x"]), eng.vector(c["y"]), eng.alloc(c["rows"])
    res = []
    for k, (alpha, beta, with_y) in enumerate(I.EPILOGUES[sr]):
        out.fill(0x5A5A5A5A, np.uint32)
        eng.spmv(sr, A, xv, yv if with_y else None, alpha, beta, out)
        res.append(out.download(np.int32))
        assert_words(res[-1], want(c, k), f"{what} alpha={alpha} beta={beta}")
    for v in (xv, yv, out):
        v.free()
    return res


# ------------------------------------------------------------------ a. sh_spmv under the five plan variants
def spmv_under_plan(eng, plan, c):
    name, sr = c["name"], c["sr"]
    builds = (1, 2) if plan.startswith("tiled") else (0,)
    outs, described = [], []
    for build in builds:
        A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], build=build) if build else \
            eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"])
        assert A.plan()[0] == plan.split("-")[0], A.describe()
        if (name, plan) in CODING:
            assert f"values={CODING[(name, plan)]}" in A.describe(), A.describe()
        if name == "clustered" and plan.startswith("tiled"):
            assert (" folded" in A.describe()) == (plan != "tiled-nofold"), A.describe()
        if name in ("wide", "dead_tiles") and plan.startswith("tiled"):
            assert int(re.search(r"tiles=(\d+)", A.describe()).group(1)) > 50, A.describe()
        if build:
            print(f"[int] {name} {SR_ID(sr)} {plan} build={build}: {A.builder()} {A.describe()}")
            described.append(A.describe())
            assert A.builder()[0] == ("device" if build == 2 else "host"), A.builder()
        outs.append(spmv_all_epilogues(eng, c, A, f"sh_spmv {name} {SR_ID(sr)} {plan} build={build}"))
        A.free()
    if len(builds) == 2:
        assert described[0] == described[1]
        for a, b in zip(*outs):
            assert_words(a, b, f"{name} {plan}: the device-built layout against the host-built one")


@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
@pytest.mark.parametrize("name", list(GENERATORS))
def test_spmv_equals_the_reference_word_for_word(eng, plan, name, sr):
    spmv_under_plan(eng, plan, data(name, sr))


def test_spmv_all_negative_max_min(eng, plan):
    """Every value, x and y below 0: empty rows, rows of 1, 16, 17, 64, 65, 4096, 4097 entries and the 70 001-entry row.  A 0
    from a padding entry, a seed or a DPP move would win the max."""
    c = data("all_negative", O.MAX_MIN_I32)
    deg = np.diff(c["rp"])
    assert set([0, 1, 16, 17, 64, 65, 4096, 4097, 70001]) <= set(deg.tolist())
    assert (c["va"] < 0).all() and (c["x"] < 0).all() and (c["y"] < 0).all() and (want(c, 0) < 0).all()
    spmv_under_plan(eng, plan, c)


@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
def test_spmv_whole_column_tiles_of_identity_x(eng, plan, sr):
    """x is the identity (0, resp. INT_MIN) in 74 of the 77 column tiles and wide words in three: the tiled plan skips a
    tile whose x words all absorb, whatever the value words are."""
    c = data("dead_tiles", sr)
    ident = 0 if sr == O.OR_AND_I32 else I.INT_MIN
    live = np.nonzero(c["x"] != ident)[0]
    assert set((live // TCOLS).tolist()) == {3, 40, 76} and (c["cols"] + TCOLS - 1) // TCOLS == 77
    spmv_under_plan(eng, plan, c)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(GENERATORS) + ["dead_tiles"])
def test_spmv_or_and_on_the_bit_blocked_layout(eng, name, mode):
    """or_and_bits = 1 (beside the ordinary plan) and 2 (alone): x becomes a bitmap and the entries lose their values at
    build time, on the host and on the device, by `!= 0` tests on the words."""
    c = data(name, O.OR_AND_I32)
    outs = []
    for build in (1, 2):
        A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], or_and_bits=mode, build=build)
        assert "or_and=bits(" in A.describe() and ("only" in A.describe()) == (mode == 2), A.describe()
        outs.append(spmv_all_epilogues(eng, c, A, f"sh_spmv {name} or_and_bits={mode} build={build}"))
        A.free()
    for a, b in zip(*outs):
        assert_words(a, b, f"{name} or_and_bits={mode}: device-built against host-built")


# ------------------------------------------------------------------ b. sh_spmm and sh_iterate_multi
@functools.lru_cache(maxsize=None)
def multi_case(sr):
    """The ragged pattern of tests/test_multi_gpu.py (one row of 20 001 entries: three long-row segments and the fix-up)."""
    rows, cols = 3001, 2500
    rp, ci, rng = ragged_csr(100 + sr, rows, cols, long_len=20_001)
    return I.case(sr, rows, cols, rp, ci, rng, width=32)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
def test_spmm_columns_equal_the_reference_and_spmv(eng, sr, width):
    c = multi_case(sr)
    assert np.diff(c["rp"]).max() == 20_001
    A = eng.upload_csr(c["rows"], c["cols"], c["rp"], c["ci"], c["va"], plan=1)
    X, Y = interleave(c["xs"][:width], np.int32), interleave(c["ys"][:width], np.int32)
    for alpha, beta, with_y in I.EPILOGUES[sr]:
        got = run_spmm(eng, sr, A, c["rows"], X, Y if with_y else None, alpha, beta)
        for j in range(width):
            y = c["ys"][j] if with_y else None
            ref = I.kernel(sr, c["rp"], c["ci"], c["va"], c["xs"][j], y, alpha, beta, c["cols"])
            assert_words(got[:, j], ref, f"sh_spmm {SR_ID(sr)} width {width} column {j} alpha={alpha} beta={beta}")
            single = run_spmv(eng, sr, A, c["rows"], c["xs"][j], y, alpha, beta)
            assert_words(got[:, j], single, f"sh_spmm against sh_spmv, {SR_ID(sr)} width {width} column {j} alpha={alpha} beta={beta}")
    A.free()


LOOP_SCALARS = {O.OR_AND_I32: (1, 1), O.MAX_MIN_I32: (I.INT_MAX, I.INT_MAX)}    # a vertex keeps what it has
CAP = 2000


@functools.lru_cache(maxsize=None)
def multi_starts(sr):
    """32 start vectors on the square ragged graph and their reference runs.  Column 1 is the identity everywhere: it is
    its own image and stops after one launch, the others need several."""
    n, rp, ci, va = I.graph("ragged", sr)
    starts = [I.start(sr, n, np.random.default_rng(700 + j), truthy=0.0005 * (1 + j)) for j in range(32)]
    starts[1] = np.full(n, 0 if sr == O.OR_AND_I32 else I.INT_MIN, np.int32)
    a, b = LOOP_SCALARS[sr]
    return starts, [I.iterate(sr, rp, ci, va, s, s, a, b, CAP) for s in starts]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
def test_iterate_multi_columns_freeze_at_their_own_launch(eng, sr, width):
    n, rp, ci, va = I.graph("ragged", sr)
    starts, ref = multi_starts(sr)
    starts, ref = starts[:width], ref[:width]
    a, b = LOOP_SCALARS[sr]
    counts = [r[1] for r in ref]
    print(f"[int] sh_iterate_multi {SR_ID(sr)} width {width}: launches of the columns {counts}")
    assert len(set(counts)) >= 2 and counts[1] == 1 and all(r[2] for r in ref)
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    X0 = interleave(starts, np.int32)
    xv, yv, sc = eng.vector(X0), eng.vector(X0), eng.alloc(n * width).fill(0)
    launches, iters, conv, _, _ = eng.iterate_multi(sr, A, xv, yv, sc, a, b, width, max_iters=CAP)
    got = xv.download(np.int32, shape=(n, width))
    for v in (xv, yv, sc):
        v.free()
    A.free()
    assert iters == counts and conv == [r[2] for r in ref] and launches == max(counts)
    for j in range(width):
        assert_words(got[:, j], ref[j][0], f"sh_iterate_multi {SR_ID(sr)} width {width} column {j}")


# ------------------------------------------------------------------ c. sh_iterate and sh_iterate_frontier
@pytest.mark.parametrize("name", ["ragged", "edges"])
@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
def test_iterate_and_frontier_equal_the_reference(eng, sr, name):
    n, rp, ci, va = I.graph(name, sr)
    if name == "edges":
        P.assert_edge_lengths(rp, ci)
    x0 = I.start(sr, n, np.random.default_rng(601))
    if sr == O.OR_AND_I32:
        marks = x0[x0 != 0]
        assert len(marks) >= 3 and not (marks == 1).any() and I.INT_MIN in marks and 0x00010000 in marks
    a, b = LOOP_SCALARS[sr]
    ref, w_it, w_conv = I.iterate(sr, rp, ci, va, x0, x0, a, b, CAP)
    assert w_conv and w_it >= 3
    ups = [dict(plan=1), dict(plan=2)] + ([dict(or_and_bits=2)] if sr == O.OR_AND_I32 else [])
    for up in ups:
        A = eng.upload_csr(n, n, rp, ci, va, **up)
        xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
        it, conv, _, _ = eng.iterate(sr, A, xv, yv, sc, a, b, max_iters=CAP)
        dense = xv.download(np.int32)
        for v in (xv, yv, sc):
            v.free()
        assert (it, conv) == (w_it, w_conv), (up, it, conv)
        assert_words(dense, ref, f"sh_iterate {SR_ID(sr)} {name} {up}")
        Fr = eng.frontier(A, rp, ci, va)
        for share in (0.0, -1.0, 1.0):
            xv, yv, sc = eng.vector(x0), eng.vector(x0), eng.alloc(n).fill(0)
            res = eng.iterate_frontier(sr, A, Fr, xv, yv, sc, a, b, max_iters=CAP, dense_share=share)
            got = xv.download(np.int32)
            for v in (xv, yv, sc):
                v.free()
            what = f"sh_iterate_frontier {SR_ID(sr)} {name} {up} dense_share {share}"
            assert res[:2] == (w_it, w_conv), (what, res[:3])
            assert_words(got, dense, what + " against sh_iterate")
            assert_words(got, ref, what)
            if share == 0.0:
                assert not any(res[2])
            if share == 1.0 and name == "ragged":
                assert 1 in res[2], (what, res[2])
        Fr.free()
        A.free()


# ------------------------------------------------------------------ d. packed bits
@pytest.mark.parametrize("words", [1, 8])
def test_bits_from_column_sets_the_bit_exactly_where_the_word_is_not_zero(eng, words):
    """The column is read four words at a time: every word of SPECIAL in every place of such a load, and in the tail n % 4."""
    rng = np.random.default_rng(41)
    k = len(I.SPECIAL)
    for tail in (1, 2, 3):
        n = 4 * 5 * k + tail
        c = I.truth_words(rng, n)
        c[5 * np.arange(k)] = I.SPECIAL                      # 5 i mod 4: all four places of a load
        c[5 * np.arange(k) + 5 * k * 2 + 2] = I.SPECIAL[::-1]
        c[n - tail:] = np.array([I.INT_MIN, 0x00010000, I.NAN_WORD], np.int32)[:tail]
        Pk = rng.integers(0, 1 << 32, (n + 3, words), dtype=np.uint64).astype(np.uint32)
        B, v, back = eng.vector(Pk), eng.vector(np.concatenate([c, [1, 1, 1]]).astype(np.int32)), eng.alloc(n + 3)
        for s in (0, 31, 32 * words - 1, 32 * words - 13):
            eng.bits_from_column(v, n, words, s, B)
            bit = np.uint32(1) << np.uint32(s % 32)
            Pk[:n, s // 32] = (Pk[:n, s // 32] & ~bit) | ((bits(c) != 0).astype(np.uint32) << np.uint32(s % 32))
            np.testing.assert_array_equal(B.download(np.uint32, shape=(n + 3, words)), Pk, err_msg=f"n {n} source {s}")
            back.fill(7, np.int32)
            eng.bits_to_column(B, n, words, s, back)
            res = back.download(np.int32)
            np.testing.assert_array_equal(res[:n], (bits(c) != 0).astype(np.int32))
            assert res[n:].tolist() == [7, 7, 7]
        for x in (B, v, back):
            x.free()


@pytest.mark.parametrize("words", [1, 8])
def test_bits_spmv_on_wide_value_words(eng, words):
    rows, cols = 3001, 2500
    rp, ci, _, rng = bits_ragged_csr(300 + words, rows, cols, long_len=20_001)
    va = I.truth_words(rng, len(ci))
    assert 0.3 < (va == 0).mean() < 0.4
    n_src = 32 * words
    X = (rng.random((cols, n_src)) < 0.002).astype(np.int32)
    Y = (rng.random((rows, n_src)) < 0.3).astype(np.int32)
    A = eng.upload_csr(rows, cols, rp, ci, va, plan=1)
    xv, yv, out = eng.vector(pack(X.T, cols, words)), eng.vector(pack(Y.T, rows, words)), eng.alloc(rows * words)
    for alpha, beta in ((1, 0), (I.INT_MIN, 0x00010000)):
        out.fill(0xdeadbeef, np.uint32)
        eng.bits_spmv(A, xv, yv if beta else None, alpha, beta, out, words)
        got = out.download(np.uint32, shape=(rows, words))
        for s in range(n_src):
            xs, ys = np.ascontiguousarray(X[:, s]), np.ascontiguousarray(Y[:, s])
            ref = I.kernel(O.OR_AND_I32, rp, ci, va, xs, ys, alpha, beta, cols)
            assert_words(column(got, s), ref, f"sh_bits_spmv words {words} source {s} alpha={alpha} beta={beta}")
            if s % words == 0:      # (the single-vector path: every source at words = 1, every eighth at 8)
                assert_words(column(got, s), run_spmv(eng, O.OR_AND_I32, A, rows, xs, ys, alpha, beta), f"sh_bits_spmv against sh_spmv, source {s}")
    for v in (xv, yv, out):
        v.free()
    A.free()


@pytest.mark.parametrize("words", [1, 8])
def test_bits_iterate_on_wide_value_words(eng, words):
    n, rp, ci, va = I.graph("ragged", O.OR_AND_I32)
    n_src = 32 * words
    verts = [0] + [int(v) for v in np.random.default_rng(43).permutation(np.arange(1, n))[:n_src - 2]] + [None]
    starts = [one_hot(n, v) for v in verts]
    ref = [I.iterate(O.OR_AND_I32, rp, ci, va, s, s, 1, 1, CAP) for s in starts]
    assert len({r[1] for r in ref}) >= 2
    A = eng.upload_csr(n, n, rp, ci, va, plan=1)
    P0 = pack(starts, n, words)
    xv, yv, sc = eng.vector(P0), eng.vector(P0), eng.alloc(n * words).fill(0)
    launches, iters, conv, _, _ = eng.bits_iterate(A, xv, yv, sc, 1, 1, words, max_iters=CAP)
    got = xv.download(np.uint32, shape=(n, words))
    for v in (xv, yv, sc):
        v.free()
    assert iters == [r[1] for r in ref] and conv == [r[2] for r in ref] and launches == max(iters)
    for s in range(n_src):
        assert_words(column(got, s), ref[s][0], f"sh_bits_iterate words {words} source {s}")
        if s % (4 * words) == 0:
            xv, yv, sc = eng.vector(starts[s]), eng.vector(starts[s]), eng.alloc(n).fill(0)
            it, cv, _, _ = eng.iterate(O.OR_AND_I32, A, xv, yv, sc, 1, 1, max_iters=CAP)
            assert (it, cv) == (iters[s], conv[s])
            assert_words(column(got, s), xv.download(np.int32), f"sh_bits_iterate against sh_iterate, source {s}")
            for v in (xv, yv, sc):
                v.free()
    A.free()


# ------------------------------------------------------------------ e. sh_bfs_graph_create and sh_bfs_levels
@pytest.mark.parametrize("name", ["ragged", "edges"])
def test_bfs_levels_take_any_non_zero_word_for_an_edge_and_a_source(eng, name):
    n, rp, ci, va = I.graph(name, O.OR_AND_I32)
    assert 0.3 < (va == 0).mean() < 0.4
    x0 = I.start(O.OR_AND_I32, n, np.random.default_rng(801), truthy=0.0005)
    assert I.INT_MIN in x0 and 0x00010000 in x0 and not (x0 == 1).any()
    ones, x1 = (va != 0).astype(np.int32), (x0 != 0).astype(np.int32)
    b = BL.oracle_bfs(n, rp, ci, ones, x1)                     # the same graph with every non-zero word replaced by 1
    assert b.E == int(((va != 0) & (ci >= 0) & (ci < n)).sum()) and b.reached > len(np.nonzero(x0)[0])
    G = eng.bfs_graph(rp, ci, va)
    assert G.edges == b.E
    for shares in (BL.TOP_DOWN, BL.BOTTOM_UP, BL.DEFAULT):
        level, parent, res = BL.run(eng, G, x0, shares)
        BL.check(b, level, parent, res, shares, f"{name} wide words")
    G.free()


# ------------------------------------------------------------------ f. the device builders
@pytest.mark.parametrize("values", ["raw", "4000 words", "255 words"])
@pytest.mark.parametrize("shape", [1, 2])
def test_device_builders_equal_the_host_builders_on_wide_words(tools, shape, values):
    rows, cols, avg, heavy, kw = BUILDER_SHAPES[shape]
    rng = np.random.default_rng(900 + shape)
    rp, ci, _ = random_matrix(rng, rows, cols, avg, heavy, **kw)
    nnz = len(ci)
    if values == "raw":
        va = I.words(rng, nnz)
    else:
        pool = I.value_pool(rng, int(values.split()[0]))
        va = pool[rng.integers(0, len(pool), nnz)]
        va[:len(pool)] = pool
    for options in (dict(fold=1), dict(fold=0), dict(fold=1, value_coding=8), dict(fold=1, value_coding=-1)):
        rc, report = compare(tools, rows, cols, rp, ci, va, **options)
        assert rc == 0, (shape, values, options, rc, report)
    lib, e = tools
    vz = np.ascontiguousarray(np.where(rng.random(nnz) < 1.0 / 3.0, 0, va), np.int32)
    buf = C.create_string_buffer(2048)
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    rc = lib.sh_debug_compare_bits_builds(e, rows, cols, nnz, _p(rp), _p(ci), _p(vz), buf, len(buf))
    assert rc == 0, (shape, values, rc, buf.value.decode())


# ------------------------------------------------------------------ g. the multi-GPU seam
@pytest.mark.parametrize("sr", SEMIRINGS, ids=SR_ID)
def test_sharded_driver_on_wide_words(sr):
    """HipLocalStep / ShardedIteration at world 1 with 3 chunks: the slotted vector layout (its padding slots, the columns
    outside the matrix), the pieces' changed flags compared on words."""
    import torch
    from sparseharness_amd.distributed import HipLocalStep, ShardedIteration, ShardPlan
    n, rp, ci, va = I.graph("ragged", sr)
    x0 = I.start(sr, n, np.random.default_rng(601))
    a, b = LOOP_SCALARS[sr]
    ref, w_it, w_conv = I.iterate(sr, rp, ci, va, x0, x0, a, b, CAP)
    torch.cuda.set_device(0)
    sp = ShardPlan(rp, ci, va, 0, 1, 3)
    final, iters, conv = ShardedIteration(sp, sr, HipLocalStep(sp, sr, 0)).run(x0, x0, a, b, 1e-4, CAP)
    assert (iters, conv) == (w_it, w_conv)
    assert_words(final, ref, f"sharded driver {SR_ID(sr)}")
