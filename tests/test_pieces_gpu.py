"""The row-piece step seam on the device: sh_spmv_step and sh_spmv_step_pieces called through the C ABI with ctypes, as
HipLocalStep.launch calls them, against tests/pieces_ref.py (the numpy model tests/test_pieces_ref.py pins) and
oracle.kernel.

  (a) mapping     every matrix x plan x semiring x geometry, report 0 and 1: the WHOLE out vector, sentinels between the
                  pieces included, equals the model; it equals sh_spmv on the same handle gathered through the geometry;
                  y is read through the mapping
  (b) reports     done words, rounds, sh_csr_piece_state, launches with different arrival counts alternating
  (c) visible     a piece copied out on a side stream the moment its word arrives equals the model
  (d) changed     the changed word in every epilogue variant: one row off at a time, y aliasing x and apart, the float
                  edge |in - out| == delta, sh_spmv_step at x_row_offset != 0
  (e) gate        a closed gate writes nothing; an open one changes nothing; the geometry changes between launches
  (f) refusals    every refusal of sh_spmv_step_pieces / sh_spmv_step, none of which moves the round

The data (values k/64 below 4.7, x in {0, 1, 3}, a third FLT_MAX for (min,+)) makes every row sum exact in float, so
every comparison is == on the bits.  Plans are forced by upload options; before a test relies on a structure (bins,
heavy rows, the bit layout) it asserts it from describe()."""
import ctypes as C
import re
import time

import numpy as np
import pytest

import pieces_ref as P
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine

pytestmark = pytest.mark.gpu

PT, MP, OA, MM = P.SEMIRINGS
F, I = (PT, MP), (OA, MM)
# name -> (upload options, the semirings the upload serves)
CFGS = {
    "stream-f": (dict(plan=1, or_and_bits=0), F),
    "tiled-f": (dict(plan=2, or_and_bits=0), F),
    "stream-i": (dict(plan=1, or_and_bits=0), I),
    "tiled-i": (dict(plan=2, or_and_bits=0), I),
    "bits1": (dict(plan=2, or_and_bits=1), I),     # (or,and) on the bit-blocked layout, (max,min) on the tiled one
    "bits2": (dict(or_and_bits=2), (OA,)),
}
DELTA = 0.25
POISON = {np.float32: np.float32(777.0), np.int32: np.int32(12345)}   # where no launch may read y / x
_halt = []   # why the module's GPU work ended early (a report that never came, a failed synchronise)


class Ctx:
    def __init__(self):
        self.eng = Engine(0)
        self.lib = abi.load()
        import torch
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.mats, self.want = {}, {}

    def mat(self, name, cfg):
        """The matrix under the configuration, uploaded once per module, with its structure read from describe()."""
        if (name, cfg) not in self.mats:
            m = P.matrix(name)
            opts, srs = CFGS[cfg]
            A = self.eng.upload_csr(m["rows"], m["cols"], m["rp"], m["ci"], P.values(m, srs[0]), **opts)
            d = A.describe()
            A.bins = int(re.search(r"bins=(\d+)", d).group(1)) if "bins=" in d else 0
            A.heavy = int(re.search(r"heavy_rows=(\d+)", d).group(1)) if "heavy_rows=" in d else 0
            A.tiled, A.bits, A.text = d.startswith("tiled"), "or_and=bits(" in d, d
            self.mats[(name, cfg)] = A
        return self.mats[(name, cfg)]

    def wanted(self, name, sr, scalars=None, yseed=2):
        """(x over the columns, y per row, row values by oracle.kernel) -- computed once and shared."""
        key = (name, sr, scalars, yseed)
        if key not in self.want:
            m = P.matrix(name)
            a, b = scalars or P.SCALARS[sr]
            x, yrow = P.vector(sr, m["cols"], 1), P.vector(sr, m["rows"], yseed)
            if sr == PT:
                assert P.exact_in_float(m, x)
            w = P.row_values(m, sr, x, yrow, a, b)
            for arr in (x, yrow, w):
                arr.setflags(write=False)
            self.want[key] = (x, yrow, w)
        return self.want[key]

    def sync(self):
        rc = self.lib.sh_engine_synchronize(self.eng.h)
        if rc:
            _halt.append(f"sh_engine_synchronize failed: {rc} {self.lib.sh_last_error(self.eng.h)}")
            pytest.fail(_halt[-1])

    def close(self):
        for A in self.mats.values():
            A.free()
        self.eng.close()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _not_halted():
    if _halt:
        pytest.fail("the module's GPU work ended at: " + _halt[0])


@pytest.fixture
def pool(ctx):
    """Device vectors of one test, freed behind it."""
    made = []

    class Pool:
        def vec(self, host):
            made.append(ctx.eng.vector(np.ascontiguousarray(host)))
            return made[-1]

        def sentinel(self, n):
            made.append(ctx.eng.alloc(n).fill(P.SENTINEL, np.uint32))
            return made[-1]

        def word(self, value):
            made.append(ctx.eng.alloc(1).fill(value, np.int32))
            return made[-1]

        def view(self, v, first, n):
            made.append(ctx.eng.wrap(v.device_ptr + 4 * first, n))
            return made[-1]
    yield Pool()
    for v in made:
        v.free()


def pieces_struct(g, report=0, gate=None):
    pc = abi.sh_row_pieces()
    pc.n_pieces, pc.piece_rows, pc.report = g.n_pieces, g.piece_rows, report
    for c in range(g.n_pieces):
        pc.element_of_piece[c] = g.elements[c]
    pc.gate = gate.device_ptr if gate is not None else None
    return pc


def scalars_of(sr, scalars=None):
    dt = P.elem_dtype(sr)
    a, b = scalars or P.SCALARS.get(sr, (0, 0))
    return np.array([a], dt), np.array([b], dt)


def step_pieces(ctx, sr, A, x, y, out, pc, flag=None, scalars=None, delta=DELTA):
    """-> (rc, *round, done words) of one sh_spmv_step_pieces; pc: a Geometry (no report, no gate) or a sh_row_pieces."""
    if isinstance(pc, P.Geometry):
        pc = pieces_struct(pc)
    a, b = scalars_of(sr, scalars)
    rnd, words = C.c_uint32(0), C.POINTER(C.c_uint32)()
    rc = ctx.lib.sh_spmv_step_pieces(ctx.eng.h, sr, A.h, x.h, None if y is None else y.h, a.ctypes.data_as(C.c_void_p),
                                     b.ctypes.data_as(C.c_void_p), out.h, None if pc is None else C.byref(pc), delta,
                                     None if flag is None else C.c_void_p(flag.device_ptr), C.byref(rnd), C.byref(words))
    return rc, rnd.value, (np.ctypeslib.as_array(words, (P.MAX_PIECES,)) if words else None)


def step(ctx, sr, A, x, y, out, offset, flag=None, scalars=None, delta=DELTA):
    a, b = scalars_of(sr, scalars)
    return ctx.lib.sh_spmv_step(ctx.eng.h, sr, A.h, x.h, None if y is None else y.h, a.ctypes.data_as(C.c_void_p),
                                b.ctypes.data_as(C.c_void_p), out.h, offset, delta,
                                None if flag is None else C.c_void_p(flag.device_ptr))


def piece_state(ctx, A):
    arr, words = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
    exp, rnd = C.c_uint32(), C.c_uint32()
    assert ctx.lib.sh_csr_piece_state(ctx.eng.h, A.h, arr, words, C.byref(exp), C.byref(rnd)) == 0
    return {"round": rnd.value, "expected": exp.value, "host_words": list(words), "arrivals": list(arr), "layout": A.text}


def expected_arrivals(ctx, A, sr):
    return min(A.bins, ctx.cus) if A.tiled and A.bins > 0 and not (sr == OA and A.bits) else 1


def in_layout(g, length, rows_words, dtype):
    """A vector of `length` words that holds one word per row at the rows' elements and poison everywhere else."""
    v = np.full(length, POISON[dtype], dtype)
    v[g.at] = rows_words
    return v


def assert_structure(name, cfg, A):
    """What the tests take the uploads for; a changed size rule fails here instead of emptying a test."""
    if name == "tiny":
        return
    if cfg == "bits2":
        assert A.bits and "only" in A.text, A.text
        return
    assert A.bits == (cfg == "bits1"), A.text
    assert A.tiled == (not cfg.startswith("stream")), A.text
    if not A.tiled:
        return
    if name == "all_heavy":
        # The builder cuts EVERY row into a bin, heavy or not, so a matrix with rows has a bin: this one has one bin
        # that holds no product.  (n_bins == 0 -- spmv_heavy_fixup, report_all_pieces behind the tiled plan -- takes a
        # matrix without rows, and such a matrix has no heavy row either.)
        assert (A.bins, A.heavy) == (1, 6) and "light=0.0M" in A.text, A.text
    if name in ("mixed", "mixed_far"):
        assert A.heavy == 7 and 2 <= A.bins, A.text
    if name == "many_bins":
        assert A.heavy == 2 and A.bins >= 280, A.text


# ------------------------------------------------------------------ (a) mapping (+ the words of (b) on the way)
@pytest.mark.parametrize("cfg", sorted(CFGS))
@pytest.mark.parametrize("name", ["tiny", "all_heavy", "mixed", "many_bins"])
def test_rows_land_on_their_elements_and_nowhere_else(ctx, pool, name, cfg):
    m, A = P.matrix(name), ctx.mat(name, cfg)
    assert_structure(name, cfg, A)
    rows, cols = m["rows"], m["cols"]
    if name == "many_bins" and A.tiled:
        assert A.bins > ctx.cus, "many_bins is meant to give a phase-2 workgroup several bins"
    if name == "mixed" and A.tiled:
        assert A.bins < ctx.cus
    for sr in CFGS[cfg][1]:
        dt = P.elem_dtype(sr)
        xc, yrow, want = ctx.wanted(name, sr)
        a, b = scalars_of(sr)
        # sh_spmv on the same handle: rows at elements 0 .. rows - 1
        xv, yv, plain = pool.vec(xc), pool.vec(yrow), pool.sentinel(rows)
        ctx.eng.spmv(sr, A, xv, yv, a[0], b[0], plain)
        ctx.sync()
        plain_bits = plain.download(np.uint32)
        assert np.array_equal(plain_bits, P.bits(want))
        for gname in (("rank1of2x3", "eight_odd") if name == "many_bins" else P.GEOMETRIES):
            g = P.named_geometry(gname, rows)
            L = max(cols, g.length)
            x = pool.vec(np.concatenate([xc, np.full(L - cols, POISON[dt], dt)]))
            y = pool.vec(in_layout(g, L, yrow, dt))      # y differs from x and is poison wherever no row lives
            out = pool.sentinel(L)
            model = P.expected_out(np.full(L, P.SENTINEL, np.uint32), P.bits(want), g.at)
            for report in (0, 1):
                before = piece_state(ctx, A)["round"]
                out.fill(P.SENTINEL, np.uint32)
                rc, rnd, words = step_pieces(ctx, sr, A, x, y, out, pieces_struct(g, report))
                assert rc == 0, ctx.lib.sh_last_error(ctx.eng.h)
                ctx.sync()
                got = out.download(np.uint32)
                bad = np.nonzero(got != model)[0]
                assert bad.size == 0, (gname, report, sr, bad[:8], got[bad[:8]], model[bad[:8]])
                assert np.array_equal(got[g.at], plain_bits)
                st = piece_state(ctx, A)
                if report:
                    assert rnd == before + 1 == st["round"]
                    assert words[:g.n_pieces].tolist() == [rnd] * g.n_pieces, (gname, st)
                    assert st["host_words"][:g.n_pieces] == [rnd] * g.n_pieces and st["arrivals"] == [0] * 8, st
                    assert st["expected"] == expected_arrivals(ctx, A, sr), st
                else:
                    assert st["round"] == before and words is None


# ------------------------------------------------------------------ (b) reports
def test_arrival_counts_alternate_on_one_matrix(ctx, pool):
    """(max,min) reports through the tiled plan's workgroups (N arrivals per piece), (or,and) through the single
    arrival behind the bit-blocked kernels: ten reporting launches, alternating, keep words == round."""
    A = ctx.mat("mixed", "bits1")
    assert_structure("mixed", "bits1", A)
    m = P.matrix("mixed")
    g = P.named_geometry("eight_odd", m["rows"])
    L = max(m["cols"], g.length)
    n_tiled = min(A.bins, ctx.cus)
    assert n_tiled > 1
    bufs = {}
    for sr in (MM, OA):
        xc, yrow, want = ctx.wanted("mixed", sr)
        bufs[sr] = (pool.vec(np.concatenate([xc, np.zeros(L - m["cols"], np.int32)])), pool.vec(in_layout(g, L, yrow, np.int32)),
                    P.expected_out(np.full(L, P.SENTINEL, np.uint32), P.bits(want), g.at))
    out = pool.sentinel(L)
    last = piece_state(ctx, A)["round"]
    for k in range(10):
        sr = (MM, OA)[k % 2]
        x, y, model = bufs[sr]
        out.fill(P.SENTINEL, np.uint32)
        rc, rnd, words = step_pieces(ctx, sr, A, x, y, out, pieces_struct(g, 1))
        assert rc == 0 and rnd == last + 1
        ctx.sync()
        st = piece_state(ctx, A)
        assert words[:8].tolist() == [rnd] * 8 and st["host_words"] == [rnd] * 8 and st["arrivals"] == [0] * 8, (k, st)
        assert st["expected"] == (n_tiled, 1)[k % 2] and st["round"] == rnd
        assert np.array_equal(out.download(np.uint32), model), k
        last = rnd


# ------------------------------------------------------------------ (d) the changed word
def chosen_rows(g, m):
    deg = np.diff(m["rp"])
    rows = dict.fromkeys(g.boundary_rows(), "piece boundary")
    rows.update({r: k for k, r in P.MIXED_CLASS_ROWS.items()} if m["name"].startswith("mixed") else {})
    assert deg[0] > 0 and deg[-1] > 0
    return rows


def changed_word_case(ctx, pool, name, cfg, sr, alias, launch, g, prev_first, x_len):
    """Shared by the pieces and the offset test.  The previous vector lives at x[prev_first + element]; the columns
    address x[0 .. cols) only, so it can be set freely.  launch(x, y, out, flag) -> rc."""
    m, A = P.matrix(name), ctx.mat(name, cfg)
    dt = P.elem_dtype(sr)
    rows, cols = m["rows"], m["cols"]
    xc = ctx.wanted(name, sr)[0]
    if alias:
        scalars = P.ALIAS_SCALARS[sr]
        key = (name, sr, "fixed")
        if key not in ctx.want:
            ctx.want[key] = P.fixed_point(m, sr, xc)
        want = ctx.want[key]
        yrow = want
        assert np.array_equal(P.bits(P.row_values(m, sr, xc, want, *scalars)), P.bits(want)), "not a fixed point"
    else:
        scalars = P.SCALARS[sr]
        _, yrow, want = ctx.wanted(name, sr)
    assert not P.expected_changed(sr, want, want, DELTA).any()
    xh = np.full(x_len, POISON[dt], dt)
    xh[:cols] = xc
    xh[prev_first + g.at] = want
    x = pool.vec(xh)
    y = x if alias == "exact" else pool.view(x, prev_first, x_len - prev_first) if alias else pool.vec(in_layout(g, x_len - prev_first, yrow, dt))
    out_len = x_len - prev_first
    out, flag = pool.sentinel(out_len), pool.word(0)
    model = P.expected_out(np.full(out_len, P.SENTINEL, np.uint32), P.bits(want), g.at)

    def run(preset):
        flag.fill(preset, np.int32)
        assert launch(x, y, out, flag, scalars) == 0, ctx.lib.sh_last_error(ctx.eng.h)
        ctx.sync()
        return int(flag.download(np.int32)[0])

    assert run(0) == 0, "prev == out and the flag was raised"
    assert np.array_equal(out.download(np.uint32), model)
    assert run(1) == 1, "a flag preset to 1 was cleared"
    raised = 0
    for r, why in chosen_rows(g, m).items():
        cell = pool.view(x, prev_first + int(g.at[r]), 1)
        off = P.perturbed(sr, want[r])
        cell.upload(np.array([off], dt))
        new = P.one_row_value(m, sr, xc, r, off, *scalars) if alias else want[r]
        expect = int(P.expected_changed(sr, [off], [new], DELTA)[0])
        assert alias or expect == 1
        got = run(0)
        assert got == expect, (r, why, float(off), float(new), int(np.diff(m["rp"])[r]))
        here = pool.view(out, int(g.at[r]), 1).download(np.uint32)
        assert here[0] == P.bits(np.array([new], dt))[0], (r, why)
        cell.upload(np.array([want[r]], dt))
        raised += expect
    assert raised >= 1, "none of the rows chosen can raise the flag under this semiring"
    assert run(0) == 0
    return x, y, out, flag, want, run


@pytest.mark.parametrize("alias", ["exact", False], ids=["y-is-x", "y-apart"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
@pytest.mark.parametrize("name", ["mixed", "all_heavy"])
def test_one_row_off_raises_the_changed_word(ctx, pool, name, cfg, alias):
    """finish_row (CSR-stream rows), spmv_long_fixup, finish_row_loaded with the previous words taken from y (y is x) or
    loaded apart, heavy_row_by_wave (also in a bin without a light row: all_heavy), bits_finish: each writes the word
    for the rows it finishes."""
    m, A = P.matrix(name), ctx.mat(name, cfg)
    assert_structure(name, cfg, A)
    g = P.named_geometry("eight_odd", m["rows"], base=m["cols"])
    for sr in CFGS[cfg][1]:
        def launch(x, y, out, flag, scalars):
            return step_pieces(ctx, sr, A, x, y, out, g, flag, scalars)[0]
        changed_word_case(ctx, pool, name, cfg, sr, alias, launch, g, 0, g.length)


@pytest.mark.parametrize("alias", ["view", False], ids=["y-is-prev", "y-apart"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_step_compares_with_the_words_at_x_row_offset(ctx, pool, cfg, alias):
    """sh_spmv_step: row r is compared with x[x_row_offset + r].  x holds cols + rows words, the previous vector at
    x_row_offset = cols; the columns of `mixed_far` leave x[0 .. rows) alone, so the words at offset 0 are free too."""
    m, A = P.matrix("mixed_far"), ctx.mat("mixed_far", cfg)
    assert_structure("mixed_far", cfg, A)
    rows, cols = m["rows"], m["cols"]
    assert m["ci"][(m["ci"] >= 0) & (m["ci"] < cols)].min() >= rows
    g = P.named_geometry("identity", rows)
    for sr in CFGS[cfg][1]:
        dt = P.elem_dtype(sr)

        def launch(x, y, out, flag, scalars, offset=cols):
            return step(ctx, sr, A, x, y, out, offset, flag, scalars)
        x, y, out, flag, want, run = changed_word_case(ctx, pool, "mixed_far", cfg, sr, alias, launch, g, cols, cols + rows)
        # the words at offset 0 differ from want, those at the offset equal it: flag 0 was seen above.
        # The reverse: want at offset 0, something else at the offset
        head = pool.view(x, 0, rows)
        tail = pool.view(x, cols, rows)
        assert P.expected_changed(sr, ctx.wanted("mixed_far", sr)[0][:rows], want, DELTA).any()
        if not alias:
            head.upload(want)
            tail.upload(np.array([P.perturbed(sr, w) for w in want], dt))
            assert run(0) == 1
            flag.fill(0, np.int32)
            assert launch(x, y, out, flag, P.SCALARS[sr], offset=0) == 0
            ctx.sync()
            assert int(flag.download(np.int32)[0]) == 0


@pytest.mark.parametrize("cfg", ["stream-f", "tiled-f"])
def test_differs_at_exactly_delta(ctx, pool, cfg):
    """delta = 0.25, prev and out multiples of 1/64: |in - out| is exact.  0.234375 below: no; 0.25: yes; NaN: yes."""
    m, A = P.matrix("mixed"), ctx.mat("mixed", cfg)
    g = P.named_geometry("eight_odd", m["rows"], base=m["cols"])
    for sr in F:
        xc, yrow, want = ctx.wanted("mixed", sr)
        xh = np.full(g.length, POISON[np.float32], np.float32)
        xh[:m["cols"]] = xc
        xh[g.at] = want
        x, y = pool.vec(xh), pool.vec(in_layout(g, g.length, yrow, np.float32))
        out, flag = pool.sentinel(g.length), pool.word(0)
        for cls in ("one_lane", "sixty_four_lanes", "heavy", "long"):
            r = P.MIXED_CLASS_ROWS[cls]
            w = want[r]
            assert 0 < w < 2 ** 18 and w * 64 == np.round(w * 64), (cls, w)
            cell = pool.view(x, int(g.at[r]), 1)
            for prev, expect in ((w + np.float32(0.234375), 0), (w - np.float32(0.234375), 0), (w + np.float32(0.25), 1),
                                 (w - np.float32(0.25), 1), (np.float32(np.nan), 1), (w, 0)):
                assert int(P.expected_changed(sr, [prev], [w], DELTA)[0]) == expect
                cell.upload(np.array([prev], np.float32))
                flag.fill(0, np.int32)
                assert step_pieces(ctx, sr, A, x, y, out, g, flag)[0] == 0
                ctx.sync()
                assert int(flag.download(np.int32)[0]) == expect, (cls, sr, float(prev), float(w))


# ------------------------------------------------------------------ (e) gate
@pytest.mark.parametrize("cfg", sorted(CFGS))
@pytest.mark.parametrize("name", ["all_heavy", "mixed"])
def test_gate(ctx, pool, name, cfg):
    m, A = P.matrix(name), ctx.mat(name, cfg)
    assert_structure(name, cfg, A)
    closed, opened = pool.word(0), pool.word(1)
    for sr in CFGS[cfg][1]:
        dt = P.elem_dtype(sr)
        xc, yrow, want = ctx.wanted(name, sr)
        geoms = [P.named_geometry(n, m["rows"]) for n in ("rank1of2x3", "eight_odd", "rank1of2x3")]
        L = max([m["cols"]] + [g.length for g in geoms])
        sent = np.full(L, P.SENTINEL, np.uint32)
        xh = np.concatenate([xc, np.full(L - m["cols"], POISON[dt], dt)])
        x = pool.vec(xh)
        ys = [pool.vec(in_layout(g, L, yrow, dt)) for g in geoms[:2]]
        out, flag = pool.sentinel(L), pool.word(0)
        g = geoms[1]
        # a closed gate: every sentinel stays, the flag stays 0
        assert step_pieces(ctx, sr, A, x, ys[1], out, pieces_struct(g, 0, closed), flag)[0] == 0
        ctx.sync()
        assert np.array_equal(out.download(np.uint32), sent) and int(flag.download(np.int32)[0]) == 0
        # an open gate: the bits of a launch without one
        assert step_pieces(ctx, sr, A, x, ys[1], out, pieces_struct(g, 0, opened), flag)[0] == 0
        ctx.sync()
        assert np.array_equal(out.download(np.uint32), P.expected_out(sent, P.bits(want), g.at))
        assert int(flag.download(np.int32)[0]) == int(P.expected_changed(sr, xh[g.at], want, DELTA).any())
        # the geometry changes between launches that nobody waits for
        outs = [pool.sentinel(L) for _ in geoms]
        for gk, o, yv in zip(geoms, outs, (ys[0], ys[1], ys[0])):
            assert step_pieces(ctx, sr, A, x, yv, o, gk)[0] == 0
        ctx.sync()
        for gk, o in zip(geoms, outs):
            assert np.array_equal(o.download(np.uint32), P.expected_out(sent, P.bits(want), gk.at)), gk.name


# ------------------------------------------------------------------ (f) refusals
def test_refusals_touch_nothing_and_do_not_count_as_rounds(ctx, pool):
    m, A = P.matrix("mixed"), ctx.mat("mixed", "tiled-f")
    Ab = ctx.mat("mixed", "bits2")
    rows, cols = m["rows"], m["cols"]
    g = P.named_geometry("eight_odd", rows, base=cols)     # (behind the columns: a piece can stick out of x)
    L = g.length
    xc, yrow, want = ctx.wanted("mixed", MP)
    x = pool.vec(np.concatenate([xc, np.full(L - cols, POISON[np.float32], np.float32)]))
    y = pool.vec(in_layout(g, L, yrow, np.float32))
    out, flag, gate = pool.sentinel(L), pool.word(0), pool.word(1)
    top = max(g.elements) + g.rows_of(int(np.argmax(g.elements)))[1]      # one past the highest element a row lives at
    assert cols < top <= L

    def pc(report=1, **change):
        s = pieces_struct(g, report, change.pop("gate", None))
        for k, v in change.items():
            if k == "element0":
                s.element_of_piece[int(np.argmax(g.elements))] = v
            else:
                setattr(s, k, v)
        return s
    EINVAL, ESHAPE = abi.SH_EINVAL, abi.SH_ESHAPE
    short = lambda v, n: pool.view(v, 0, n)   # noqa: E731
    cases = [
        ("NULL pieces", EINVAL, dict(pc=None)),
        ("no pieces", EINVAL, dict(pc=pc(n_pieces=0))),
        ("nine pieces", EINVAL, dict(pc=pc(n_pieces=9))),
        ("pieces of no rows", EINVAL, dict(pc=pc(piece_rows=0))),
        ("pieces that do not cover the rows", EINVAL, dict(pc=pc(n_pieces=7))),
        ("a negative element", ESHAPE, dict(pc=pc(element0=-1))),
        ("a piece past the end of out", ESHAPE, dict(out=short(out, top - 1))),
        ("a piece past the end of x", ESHAPE, dict(x=short(x, top - 1))),
        ("a piece past the end of y", ESHAPE, dict(y=short(y, top - 1))),
        ("x shorter than the columns", ESHAPE, dict(x=short(x, cols - 1))),
        ("out aliasing x", EINVAL, dict(out=x)),
        ("a gated launch that reports", EINVAL, dict(pc=pc(gate=gate))),
        ("y NULL under an epilogue that reads it", EINVAL, dict(y=None)),
        ("an unknown semiring", EINVAL, dict(sr=9)),
        ("a bits-only matrix under (max,min)", EINVAL, dict(sr=MM, A=Ab)),
    ]
    before = {id(M): piece_state(ctx, M)["round"] for M in (A, Ab)}
    for what, code, change in cases:
        args = dict(sr=MP, A=A, x=x, y=y, out=out, pc=pc())
        args.update(change)
        rc, rnd, words = step_pieces(ctx, args["sr"], args["A"], args["x"], args["y"], args["out"], args["pc"], flag)
        assert rc == code, (what, rc, ctx.lib.sh_last_error(ctx.eng.h))
        assert ctx.lib.sh_last_error(ctx.eng.h), what
        assert rnd == 0 and words is None, what
    rc, _, _ = step_pieces(ctx, MP, A, x, y, out, pc(gate=gate), flag)
    assert rc == EINVAL and b"gated launch cannot report" in ctx.lib.sh_last_error(ctx.eng.h)
    # sh_spmv_step
    xs, outs = pool.vec(np.zeros(cols + rows, np.float32)), pool.sentinel(rows)
    ysr = pool.vec(yrow)
    for off in (-1, cols + 1, cols + rows):
        assert step(ctx, MP, A, xs, ysr, outs, off, flag) == ESHAPE, off
    ctx.sync()
    assert np.array_equal(out.download(np.uint32), np.full(L, P.SENTINEL, np.uint32))
    assert np.array_equal(outs.download(np.uint32), np.full(rows, P.SENTINEL, np.uint32))
    assert int(flag.download(np.int32)[0]) == 0
    assert np.array_equal(P.bits(x.download(np.float32)[:cols]), P.bits(xc))
    for M in (A, Ab):
        assert piece_state(ctx, M)["round"] == before[id(M)]
    # the good call after them: previous + 1
    rc, rnd, words = step_pieces(ctx, MP, A, x, y, out, pc(), flag)
    assert rc == 0 and rnd == before[id(A)] + 1
    ctx.sync()
    assert words[:8].tolist() == [rnd] * 8
    assert np.array_equal(out.download(np.uint32), P.expected_out(np.full(L, P.SENTINEL, np.uint32), P.bits(want), g.at))


# ------------------------------------------------------------------ (c) visible when reported (last: it may end the module)
def test_a_reported_piece_is_visible_while_the_launch_runs(ctx):
    """Torch-owned buffers on an engine that borrows torch's stream, as HipLocalStep has them.  The host polls word c
    (30 s at most, as wait_piece), and the moment it reaches *round copies piece c out on a side stream and waits for
    that stream only, as the driver's gloo branch does.  Recorded, not asserted: for how many pieces the LAST word was
    still below *round at that moment (whether the launch is still running then is timing nobody has measured)."""
    import torch
    torch.cuda.set_device(0)
    m = P.matrix("many_bins")
    rows, cols = m["rows"], m["cols"]
    eng = Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    A = eng.upload_csr(rows, cols, m["rp"], m["ci"], m["vf"], plan=2, or_and_bits=0)
    try:
        d = A.describe()
        assert d.startswith("tiled") and int(re.search(r"bins=(\d+)", d).group(1)) > ctx.cus, d
        g = P.named_geometry("eight_odd", rows)
        L = max(cols, g.length)
        xc, yrow, want = ctx.wanted("many_bins", MP)
        dev = torch.device("cuda", 0)
        x_t = torch.from_numpy(np.concatenate([xc, np.full(L - cols, POISON[np.float32], np.float32)])).to(dev)
        y_t = torch.from_numpy(in_layout(g, L, yrow, np.float32)).to(dev)
        out_t = torch.from_numpy(np.full(L, P.SENTINEL, np.uint32).view(np.float32).copy()).to(dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        x, y, out = (eng.wrap(t.data_ptr(), L) for t in (x_t, y_t, out_t))
        a, b = scalars_of(MP)
        pc = pieces_struct(g, 1)
        rnd, words_p = C.c_uint32(0), C.POINTER(C.c_uint32)()
        rc = ctx.lib.sh_spmv_step_pieces(eng.h, MP, A.h, x.h, y.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                         out.h, C.byref(pc), DELTA, None, C.byref(rnd), C.byref(words_p))
        assert rc == 0, ctx.lib.sh_last_error(eng.h)
        words = np.ctypeslib.as_array(words_p, (P.MAX_PIECES,))
        still_running, pieces = 0, []
        for c in range(g.n_pieces):
            t0 = time.perf_counter()
            while words[c] < rnd.value:
                if time.perf_counter() - t0 > 30.0:
                    arr, hw = (C.c_uint32 * 8)(), (C.c_uint32 * 8)()
                    exp, r2 = C.c_uint32(), C.c_uint32()
                    ctx.lib.sh_csr_piece_state(eng.h, A.h, arr, hw, C.byref(exp), C.byref(r2))
                    _halt.append(f"piece {c} of round {rnd.value} was not reported within 30 s: round {r2.value}, expected "
                                 f"{exp.value}, host words {list(hw)}, arrivals {list(arr)}, {d}")
                    pytest.fail(_halt[-1])
            still_running += int(words[g.n_pieces - 1] < rnd.value)
            lo, n = g.rows_of(c)
            with torch.cuda.stream(side):
                piece = out_t[g.elements[c]:g.elements[c] + n].to("cpu", non_blocking=True)
                side.synchronize()
            pieces.append((lo, n, piece.numpy().view(np.uint32).copy()))
        torch.cuda.current_stream().synchronize()
        print(f"\n[pieces] {still_running} of {g.n_pieces} pieces were copied out while the last word was still below the round")
        for lo, n, got in pieces:
            assert np.array_equal(got, P.bits(want)[lo:lo + n]), lo
        full = out_t.cpu().numpy().view(np.uint32)
        assert np.array_equal(full, P.expected_out(np.full(L, P.SENTINEL, np.uint32), P.bits(want), g.at))
        for v in (x, y, out):
            v.free()
    finally:
        if not _halt:
            torch.cuda.synchronize()
            A.free()
            eng.close()
