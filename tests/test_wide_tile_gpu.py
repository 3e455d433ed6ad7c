"""The WIDE x tile of the tiled plan on the GPU (SH_TILE_COLS=wide): phase 1's wide instantiations -- 16-bit column
codes, fold flags from fmask[], the longer staging loop -- against the oracle, through both builders.  Weights and x are
small integers, so every sum is exact and results are compared for equal bits; one case with real values is held to the
float64 bound of tests/float_ref.py.  tests/test_wide_tile_cpu.py checks the layout itself without a GPU."""
import re

import numpy as np
import pytest

import float_ref as F
from oracle import oracle as O
from sparseharness_amd.engine import Engine
from test_builder_gpu import compare, tools   # noqa: F401  (tools: the fixture that builds and loads the tools build)

pytestmark = pytest.mark.gpu

SEMIRINGS = [O.PLUS_TIMES_F32, O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32]
EPILOGUE = {O.PLUS_TIMES_F32: (1.0, 0.5), O.MIN_PLUS_F32: (0.0, 0.0), O.OR_AND_I32: (1, 1), O.MAX_MIN_I32: (1, 1)}
FLT_MAX = np.float32(np.finfo(np.float32).max)
ROWS = 5000


@pytest.fixture(scope="module")
def eng():
    with Engine(0) as e:
        yield e


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("SH_TILE_COLS", "wide")


@pytest.fixture(scope="module")
def W(eng):
    """The wide width, as a layout reports it."""
    mp = pytest.MonkeyPatch()
    mp.setenv("SH_TILE_COLS", "wide")
    try:
        A = eng.upload_csr(1, 5, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1], np.float32), plan=2)
        w = int(re.search(r" tile=(\d+) ", A.describe()).group(1))
        A.free()
    finally:
        mp.undo()
    assert 32768 < w <= 65528 and w % 8 == 0
    return w


@pytest.fixture(scope="module")
def mat(W):
    """5000 x (2 W + 1001): three tiles, the last one partial; degrees 1..40, one heavy row (600 entries: >= 512 and
    >= 8 per tile) and one row of two entries in each tile; weights 1..16.  The oracle's results are computed once."""
    rng = np.random.default_rng(2024)
    cols = 2 * W + 1001
    deg = 1 + np.arange(ROWS) % 40
    deg[1234] = 600
    deg[77] = 6
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = rng.integers(0, cols, int(rp[-1])).astype(np.int32)
    ci[rp[77]:rp[78]] = [5, 40_000, W + 5, W + 40_000, 2 * W + 5, 2 * W + 900]
    ci[:6] = [0, 32767, 32768, W - 1, W, cols - 1]
    va = rng.integers(1, 17, len(ci)).astype(np.float32)
    m = dict(rows=ROWS, cols=cols, rp=rp, ci=ci, va=va, gold={})
    m["x"] = (1 + np.arange(cols) % 7).astype(np.float32)
    m["y"] = (np.arange(ROWS) % 5).astype(np.float32)
    return m


def operands(m, sr, dead_tile=None, W=0):
    """values, x, y of the main matrix for a semiring; dead_tile: that tile of x holds the semiring's absorbing word."""
    integer = sr in (O.OR_AND_I32, O.MAX_MIN_I32)
    dt = np.int32 if integer else np.float32
    vals = m["va"].astype(dt)
    x = (np.arange(m["cols"]) % 3 == 0).astype(dt) if sr == O.OR_AND_I32 else m["x"].astype(dt)
    if dead_tile is not None:
        x = x.copy()
        x[dead_tile * W:(dead_tile + 1) * W] = {O.MIN_PLUS_F32: FLT_MAX, O.OR_AND_I32: 0}[sr]
    return vals, x, m["y"].astype(dt)


def gold(m, sr, dead_tile=None, W=0):
    key = (sr, dead_tile)
    if key not in m["gold"]:
        vals, x, y = operands(m, sr, dead_tile, W)
        m["gold"][key] = O.kernel(sr, m["rp"], m["ci"], vals, x, y, *EPILOGUE[sr])
        m["gold"][key].setflags(write=False)
    return m["gold"][key]


def run(eng, sr, A, x, y, misalign=False):
    dt = O.elem_dtype(sr)
    if misalign:   # x at a base 4 bytes past an allocation: phase 1's fallback staging loop
        base = eng.vector(np.concatenate([np.zeros(1, dt), x]))
        xv = eng.wrap(base.device_ptr + 4, len(x))
        assert xv.device_ptr % 16 == 4
    else:
        base, xv = None, eng.vector(x)
    yv, out = eng.vector(y), eng.alloc(len(y))
    eng.spmv(sr, A, xv, yv, *EPILOGUE[sr], out)
    got = out.download(dt)
    for v in (xv, yv, out, base):
        if v is not None:
            v.free()
    return got


def same_bits(got, want, what):
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=what)


@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("sr", SEMIRINGS)
def test_all_semirings_both_builders(eng, mat, W, sr, build):
    vals, x, y = operands(mat, sr)
    A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], vals, plan=2, build=build)
    d = A.describe()
    assert A.builder()[0] == ("host", "device")[build - 1] and f"tiles=3 tile={W} " in d and "heavy_rows=1 " in d and " folded" in d, d
    assert int(re.search(r"bins=(\d+)", d).group(1)) >= 3, d
    same_bits(run(eng, sr, A, x, y), gold(mat, sr), d)
    A.free()


@pytest.mark.parametrize("build", [1, 2])
@pytest.mark.parametrize("sr", [O.MIN_PLUS_F32, O.OR_AND_I32])
def test_dead_tile_in_the_middle(eng, mat, W, sr, build):
    """Tile 1 of x all absorbing: phase 1 writes none of its products (obase differences are not needed: the pieces are
    marked dead by tiled_mark_dead), phase 2 reads the identity group instead; then a live x through the same matrix."""
    vals, x, y = operands(mat, sr, 1, W)
    A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], vals, plan=2, build=build)
    same_bits(run(eng, sr, A, x, y), gold(mat, sr, 1, W), A.describe())
    _, x_live, _ = operands(mat, sr)
    same_bits(run(eng, sr, A, x_live, y), gold(mat, sr), A.describe())
    A.free()


def test_builders_agree_byte_for_byte(tools, mat, W):
    for options in (dict(fold=1), dict(fold=0), dict(fold=1, value_coding=8), dict(fold=1, value_coding=-1)):
        rc, report = compare(tools, mat["rows"], mat["cols"], mat["rp"], mat["ci"], mat["va"], **options)
        assert rc == 0, (options, rc, report)


@pytest.mark.parametrize("coding,want", [(0, "dict4(16)"), (8, "dict8(17)"), (-1, "raw")])
def test_each_value_coding_aligned_and_misaligned(eng, mat, W, coding, want):
    sr = O.PLUS_TIMES_F32
    vals, x, y = operands(mat, sr)
    A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], vals, plan=2, value_coding=coding)
    d = A.describe()
    assert f"values={want} " in d and f" tile={W} " in d, d
    same_bits(run(eng, sr, A, x, y), gold(mat, sr), d)
    same_bits(run(eng, sr, A, x, y, misalign=True), gold(mat, sr), d + " (x misaligned)")
    A.free()


def test_two_byte_codes_stay_narrow(eng, mat, W):
    sr = O.PLUS_TIMES_F32
    _, x, y = operands(mat, sr)
    vals = (1 + np.arange(len(mat["ci"])) % 300).astype(np.float32)          # 300 distinct words; sums stay below 2^24
    A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], vals, plan=2)
    d = A.describe()
    assert "values=dict16(301) " in d and "tile=" not in d and f"tiles={-(-mat['cols'] // 32760)} " in d, d
    same_bits(run(eng, sr, A, x, y), O.kernel(sr, mat["rp"], mat["ci"], vals, x, y, *EPILOGUE[sr]), d)
    A.free()


def test_real_values_within_the_float64_bound(eng, mat, W):
    rng = np.random.default_rng(5)
    va = F.wide_range(rng, len(mat["ci"]))
    x = F.wide_range(rng, mat["cols"])
    y = F.wide_range(rng, mat["rows"])
    dot, mag, n = F.exact_rows(mat["rp"], mat["ci"], va, x, mat["cols"])
    A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], va, plan=2)
    assert "values=raw " in A.describe() and f" tile={W} " in A.describe(), A.describe()
    xv, yv, out = eng.vector(x), eng.vector(y), eng.alloc(mat["rows"])
    for alpha, beta in ((1.0, 0.0), (-0.75, 1.5)):
        eng.spmv(O.PLUS_TIMES_F32, A, xv, yv, alpha, beta, out)
        F.assert_within(out.download(), dot, mag, n, alpha, y, beta, what=f"wide tile alpha={alpha:g} beta={beta:g}")
    for v in (xv, yv, out):
        v.free()
    A.free()


@pytest.mark.parametrize("build", [1, 2])
def test_free_returns_the_device_memory(eng, mat, W, build):
    sr = O.PLUS_TIMES_F32
    vals, x, y = operands(mat, sr)

    def once():
        A = eng.upload_csr(mat["rows"], mat["cols"], mat["rp"], mat["ci"], vals, plan=2, build=build)
        assert f" tile={W} " in A.describe()
        got = run(eng, sr, A, x, y)
        A.free()
        eng.synchronize()
        return got

    once()                                   # (the first upload of a kind loads code objects and the builders' scratch)
    before = eng.max_alloc()
    same_bits(once(), gold(mat, sr), "upload, launch, free")
    assert eng.max_alloc() == before
