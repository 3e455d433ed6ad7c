"""What keeps tests/test_int_gpu.py honest, checked without a GPU:
  1. tests/int_ref.py (numpy, from the definition) and the sequential C oracle agree word for word on every seeded
     input, both integer semirings, every epilogue, the five golden matrices and the reference's own SCC result -- so
     an exact demand made of the engine rests on the semiring and not on one implementation of it,
  2. the inputs can see each way a kernel may leave the integer view: every mutant of the reference below (a float-view
     compare, a compare by subtraction, an unsigned compare, a trip through float32, 16-bit truncation, a 0 seed, a 0
     from padding; for (or,and) a float-view or 16-bit test for zero, a bitwise AND, the OR of the words) changes at
     least 1 % of the non-empty rows of `ragged`.  That is a property of the inputs, not of the engine.
"""
import functools

import numpy as np
import pytest

import int_ref as I
from conftest import MATRICES, golden, mtx
from oracle import oracle as O

SEMIRINGS = [O.OR_AND_I32, O.MAX_MIN_I32]


def clustered_matrix(n=60_000, seed=11):
    # imported late, as tests/test_minplus_ref.py does: that module opens no device by itself (its Engine is a fixture)
    from test_parity_gpu import clustered_matrix as cm
    return cm(n, seed)


GENERATORS = I.generators(clustered_matrix)


@functools.lru_cache(maxsize=None)
def data(name, sr):
    return GENERATORS[name](sr)


def test_semiring_ids_and_pool():
    assert (I.OR_AND, I.MAX_MIN, I.INT_MIN, I.INT_MAX) == (O.OR_AND_I32, O.MAX_MIN_I32, O.INT_MIN, O.INT_MAX)
    must = [0, 1, 0xFFFFFFFF, 2, 0x80000000, 0x80000001, 0x7FFFFFFF, 0x7FFFFFFE, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
            0x7F800001, 0xFF800001, 0x00000001, 0x007FFFFF, 0x807FFFFF, 0x7F7FFFFF, 0x00010000, 0xFFFF0000, 0x0000FFFF,
            0x01000000, 0x01000001, (-(1 << 24)) & 0xFFFFFFFF, (-(1 << 24) - 1) & 0xFFFFFFFF]
    assert set(must) <= set(I.bits(I.SPECIAL).tolist())
    w = I.words(np.random.default_rng(1), 300_000)
    special = np.isin(w, I.SPECIAL)
    assert 0.32 < special.mean() < 0.35 and set(I.SPECIAL.tolist()) <= set(w.tolist())
    rest = I.bits(w[~special]).astype(np.float64)
    assert abs(rest.mean() / 2 ** 32 - 0.5) < 0.01 and rest.min() < 2 ** 20 and rest.max() > 2 ** 32 - 2 ** 20   # uniform over all words
    assert (I.negative_words(np.random.default_rng(2), 1000) < 0).all()
    assert I.i32(0x80000001) == I.INT_MIN + 1 and I.i32(-1) == -1 and I.i32(0x7FC00000) == 0x7FC00000
    for distinct in (16, 255, 4000):
        pool = I.value_pool(np.random.default_rng(distinct), distinct)
        assert len(np.unique(pool)) == distinct and {0, I.INT_MIN, I.NAN_WORD} <= set(pool.tolist())


# ------------------------------------------------------------------ 1. the two references agree
@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("name", list(GENERATORS))
def test_reference_equals_the_oracle_on_every_input(name, sr):
    c = data(name, sr)
    if sr == O.OR_AND_I32:
        for v in (c["x"], c["va"]):
            assert 0.3 < (v == 0).mean() < 0.4, name
    else:
        assert not np.isin(c["x"], [0, 1]).mean() > 0.05 and (c["va"] < 0).any() and (c["va"] > 2 ** 24).any()
    if name == "ragged":
        assert (c["ci"] < 0).any() and (c["ci"] >= c["cols"]).any() and (np.diff(c["rp"]) == 0).any()
    for alpha, beta, with_y in I.EPILOGUES[sr]:
        assert I.reads_y(sr, beta) == with_y
        want = O.kernel(sr, c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, vlength=c["cols"])
        got = I.kernel(sr, c["rp"], c["ci"], c["va"], c["x"], c["y"] if with_y else None, alpha, beta, c["cols"])
        np.testing.assert_array_equal(I.bits(got), I.bits(want), err_msg=f"{name} alpha={alpha} beta={beta}")


@pytest.mark.parametrize("sr", SEMIRINGS)
def test_reference_does_not_depend_on_the_stored_order(sr):
    c = data("ragged", sr)
    rng = np.random.default_rng(7)
    row_of = I.rows_of_entries(c["rp"])
    perm = np.lexsort((rng.random(len(row_of)), row_of))
    alpha, beta, _ = I.EPILOGUES[sr][2]
    a = I.kernel(sr, c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, c["cols"])
    b = O.kernel(sr, c["rp"], c["ci"][perm], c["va"][perm], c["x"], c["y"], alpha, beta, vlength=c["cols"])
    np.testing.assert_array_equal(I.bits(a), I.bits(b))


def test_an_empty_row_gives_the_identity_through_the_epilogue():
    rp = np.array([0, 0, 1], np.int32)
    ci, va = np.array([5], np.int32), np.array([9], np.int32)       # the one entry lies outside [0, 2)
    x, y = np.array([3, 4], np.int32), np.array([-8, I.INT_MIN], np.int32)
    for sr in SEMIRINGS:
        for alpha, beta, with_y in I.EPILOGUES[sr]:
            got = I.kernel(sr, rp, ci, va, x, y if with_y else None, alpha, beta, 2)
            np.testing.assert_array_equal(got, O.kernel(sr, rp, ci, va, x, y, alpha, beta, vlength=2))
    assert I.kernel(I.MAX_MIN, rp, ci, va, x, None, I.INT_MAX, I.INT_MIN, 2).tolist() == [I.INT_MIN, I.INT_MIN]
    assert I.kernel(I.MAX_MIN, rp, ci, va, x, y, 7, -3, 2).tolist() == [-8, I.INT_MIN]
    assert I.kernel(I.OR_AND, rp, ci, va, x, y, 1, 5, 2).tolist() == [1, 1]      # INT_MIN is a non-zero y


@pytest.mark.parametrize("sr", SEMIRINGS)
@pytest.mark.parametrize("name", ["ragged", "edges"])
def test_iterate_equals_the_oracle_on_the_graphs(name, sr):
    n, rp, ci, va = I.graph(name, sr)
    x0 = I.start(sr, n, np.random.default_rng(601))
    scalars = ((1, 1), (1, 0)) if sr == O.OR_AND_I32 else ((I.INT_MAX, I.INT_MAX), (I.INT_MAX, I.INT_MIN))
    for (a, b), cap in zip(scalars, (2000, 5)):
        want, w_it, w_conv = O.iterate(sr, rp, ci, va, x0, x0, a, b, 1e-4, cap)
        got, it, conv = I.iterate(sr, rp, ci, va, x0, x0, a, b, cap)
        assert (it, conv) == (w_it, w_conv)
        np.testing.assert_array_equal(I.bits(got), I.bits(want))
        if cap == 2000:
            assert conv and it >= 3, (name, sr, it)


def test_reference_equals_the_oracle_on_the_golden_matrices(matrix_name):
    rows, cols, _, rp, ci, va = O.mm_load(mtx(matrix_name), elem_is_int=True)
    rng = np.random.default_rng(11)
    for sr in SEMIRINGS:
        draw = I.truth_words if sr == O.OR_AND_I32 else I.words
        x, y = draw(rng, cols), I.words(rng, rows)
        for vals in (va, draw(rng, len(va))):
            for alpha, beta, with_y in I.EPILOGUES[sr]:
                want = O.kernel(sr, rp, ci, vals, x, y, alpha, beta, vlength=cols)
                np.testing.assert_array_equal(I.bits(I.kernel(sr, rp, ci, vals, x, y if with_y else None, alpha, beta, cols)), I.bits(want))
        if rows == cols:
            x0 = O.initial_vector(sr, rows)
            y0 = x0 if sr == O.OR_AND_I32 else np.full(rows, O.INT_MIN, np.int32)
            a, b = (1, 0) if sr == O.OR_AND_I32 else (O.INT_MAX, O.INT_MIN)
            want, w_it, w_conv = O.iterate(sr, rp, ci, va, x0, y0, a, b, 1e-4, 300)
            got, it, conv = I.iterate(sr, rp, ci, va, x0, y0, a, b, 300)
            assert (it, conv) == (w_it, w_conv)
            np.testing.assert_array_equal(got, want)


def test_scc_labels_of_the_reference():
    """The reference's own (max,min) run: matrix5 normalised for SCC, x0 = the vertex ids, y0 = INT_MIN."""
    g = golden("matrix5")
    rows, cols, _, rp, ci, va = O.mm_load(mtx("matrix5"), elem_is_int=True, normalise=O.NORM_SCC)
    x0, y0 = O.initial_vector(O.MAX_MIN_I32, rows), np.full(rows, O.INT_MIN, np.int32)
    got, it, conv = I.iterate(I.MAX_MIN, rp, ci, va, x0, y0, O.INT_MAX, O.INT_MIN, 300)
    np.testing.assert_array_equal(got, g["scc_final"])
    assert [it, int(conv)] == g["scc_meta"].tolist()


# ------------------------------------------------------------------ 2. mutants of the reference
def f32_view(v):
    return np.ascontiguousarray(v.astype(np.int32)).view(np.float32)


def lt_float_view(a, b):
    with np.errstate(invalid="ignore"):
        return f32_view(a) < f32_view(b)                      # -0.0 == +0.0, NaN unordered, negative order reversed


def lt_subtraction(a, b):
    return (a - b).astype(np.int32) < 0                       # wraps at |a - b| >= 2^31


def lt_unsigned(a, b):
    return (a & 0xFFFFFFFF) < (b & 0xFFFFFFFF)


def lt_through_float(a, b):
    return a.astype(np.float32) < b.astype(np.float32)        # the VALUE rounded to 24 bits


def lt_exact(a, b):
    return a < b


def max_min_with(lt, c, alpha, beta, seed=I.INT_MIN, values=None, pad=None):
    """I.kernel for (max,min) with `a < b` replaced by lt(a, b) in min and max (a < b ? a : b, a > b ? a : b as in the
    semiring's text), the accumulator seeded with `seed`, and `pad` = (x, a) of one further entry per row.  Rows are
    reduced entry by entry in stored order (a compare that is no order makes the result depend on it), all rows in step."""
    rp = np.asarray(c["rp"], np.int64)
    a = np.asarray(c["va"] if values is None else values).astype(np.int64)
    prod_x = I.gather(c["x"], c["ci"], c["cols"], I.INT_MIN)
    prod = np.where(lt(prod_x, a), prod_x, a)
    deg = np.diff(rp)
    acc = np.full(len(deg), seed, np.int64)
    order = np.argsort(-deg, kind="stable")                   # rows by falling length: the rows still running are a prefix
    sdeg = deg[order]
    for k in range(int(sdeg[0]) if len(sdeg) else 0):
        live = order[:int(np.searchsorted(-sdeg, -k, side="left"))]   # rows with more than k entries
        p = prod[rp[live] + k]
        acc[live] = np.where(lt(p, acc[live]), acc[live], p)  # acc > p ? acc : p
    if pad is not None:
        px, pa = np.int64(pad[0]), np.int64(pad[1])
        p = np.full(len(deg), px if lt(np.array([px]), np.array([pa]))[0] else pa, np.int64)
        acc = np.where(lt(p, acc), acc, p)
    al, be = np.full(len(deg), I.i32(alpha), np.int64), np.full(len(deg), I.i32(beta), np.int64)
    m1 = np.where(lt(acc, al), acc, al)
    y = np.asarray(c["y"]).astype(np.int64)
    m2 = np.where(lt(y, be), y, be) if I.reads_y(I.MAX_MIN, beta) else np.full(len(deg), I.INT_MIN, np.int64)
    return np.where(lt(m2, m1), m1, m2).astype(np.int32)


MAX_MIN_MUTANTS = {
    "float-view compare": dict(lt=lt_float_view),
    "compare by int32 subtraction": dict(lt=lt_subtraction),
    "unsigned compare": dict(lt=lt_unsigned),
    "through float32 before comparing": dict(lt=lt_through_float),
    "values cut to their low 16 bits": dict(lt=lt_exact, low16=True),
    "accumulator starts at 0": dict(lt=lt_exact, seed=0),
    # the layout's padding word is 0 in both places: a padding entry whose x is that word instead of the semiring's identity
    "a padding entry (x = 0, a = 0) per row": dict(lt=lt_exact, pad=(0, 0)),
}


def shorten(c, longest=4097):
    """`c` without the rows above `longest` entries (the mutants walk a row entry by entry)."""
    deg = np.diff(c["rp"])
    keep_row = deg <= longest
    keep = np.repeat(keep_row, deg)
    out = dict(c)
    out["rp"] = np.concatenate([[0], np.cumsum(np.where(keep_row, deg, 0))]).astype(np.int32)
    out["ci"], out["va"] = c["ci"][keep], c["va"][keep]
    return out


@pytest.mark.parametrize("mutant", list(MAX_MIN_MUTANTS))
def test_max_min_mutants_change_one_row_in_a_hundred(mutant):
    c = shorten(data("ragged", O.MAX_MIN_I32))
    full = np.diff(c["rp"]) > 0
    kw = dict(MAX_MIN_MUTANTS[mutant])
    if kw.pop("low16", False):
        kw["values"] = c["va"] & 0xFFFF
    for alpha, beta, with_y in I.EPILOGUES[I.MAX_MIN][:1]:      # the row results themselves
        true = I.kernel(I.MAX_MIN, c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, c["cols"])
        np.testing.assert_array_equal(max_min_with(lt_exact, c, alpha, beta), true)      # the walk itself is right
        got = max_min_with(alpha=alpha, beta=beta, c=c, **kw)
        share = float((I.bits(got) != I.bits(true))[full].mean())
        print(f"[int ref] (max,min) {mutant}, alpha={alpha} beta={beta}: {share:.4f} of {int(full.sum())} non-empty rows change")
        assert full.sum() > 4000 and share >= 0.01


def or_and_with(c, alpha, beta, truth=lambda v: v != 0, mul=None, as_words=False):
    """I.kernel for (or,and) with `v != 0` replaced by truth(v), the product by mul(x, a) (-> bool), or the result by
    the OR of the product words instead of 0 / 1."""
    a = np.asarray(c["va"]).astype(np.int64)
    xv = I.gather(c["x"], c["ci"], c["cols"], 0)
    if as_words:
        prod = np.where((xv != 0) & (a != 0), (xv | a) & 0xFFFFFFFF, 0)
        dot = I.reduce_rows(np.bitwise_or, c["rp"], prod, 0)
    else:
        prod = mul(xv, a) if mul is not None else truth(xv) & truth(a)
        dot = I.reduce_rows(np.logical_or, c["rp"], prod, False).astype(np.int64)
    al, be = np.int64(I.i32(alpha)), np.int64(I.i32(beta))
    y = np.asarray(c["y"]).astype(np.int64)
    if as_words:
        r1 = np.where(alpha != 0, dot, 0)
        r2 = np.where((y != 0) & (be != 0), 1, 0) if I.reads_y(I.OR_AND, beta) else 0
        return (r1 | r2).astype(np.uint32).view(np.int32)
    r1 = truth(dot) & bool(truth(np.array([al]))[0])
    r2 = truth(y) & bool(truth(np.array([be]))[0]) if I.reads_y(I.OR_AND, beta) else False
    return (r1 | r2).astype(np.int32)


OR_AND_MUTANTS = {
    "float-view != 0": dict(truth=lambda v: f32_view(v) != 0),                 # -0.0 counts as zero
    "truth of the low 16 bits": dict(truth=lambda v: (v & 0xFFFF) != 0),
    "x & a bitwise": dict(mul=lambda x, a: (x & a) != 0),
    "the OR of the words, not 0 / 1": dict(as_words=True),
}


@pytest.mark.parametrize("mutant", list(OR_AND_MUTANTS))
def test_or_and_mutants_change_one_row_in_a_hundred(mutant):
    c = data("ragged", O.OR_AND_I32)
    full = np.diff(c["rp"]) > 0
    for alpha, beta, with_y in I.EPILOGUES[I.OR_AND][:1]:       # the row results themselves
        true = I.kernel(I.OR_AND, c["rp"], c["ci"], c["va"], c["x"], c["y"], alpha, beta, c["cols"])
        np.testing.assert_array_equal(or_and_with(c, alpha, beta), true)
        got = or_and_with(c, alpha, beta, **OR_AND_MUTANTS[mutant])
        share = float((I.bits(got) != I.bits(true))[full].mean())
        print(f"[int ref] (or,and) {mutant}, alpha={alpha} beta={beta}: {share:.4f} of {int(full.sum())} non-empty rows change")
        assert full.sum() > 4000 and share >= 0.01
