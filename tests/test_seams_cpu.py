"""From the references alone: every input of tests/seam_shapes.py takes exactly the number of launches, steps or rounds
it is built for, so tests/test_seams_gpu.py aims at the batch seams it claims to aim at.  No device is needed."""
import numpy as np
import pytest

import int_ref as I
import minplus_ref as M
import scc_ref
import seam_shapes as S
import sssp_ref
from oracle import oracle as O

SEMIRINGS = (S.PT, S.MP, S.OA, S.MM)


def test_the_seam_sets_straddle_every_batch_end():
    for seam in (8, 16, 24):   # (launch 23 is reached as the cap 24 - 1)
        assert {seam, seam + 1} <= set(S.S8) and seam - 1 in set(S.S8) | {c for L in S.S8 for c in S.caps_for(L)}
    for seam in (8, 24, 56, 88):                        # 8, + 16, + 32, + 32
        assert {seam - 1, seam, seam + 1} <= set(S.S32)
    assert set(S.S32_TRUSS) == set(S.S32) - {87, 88, 89}
    assert {1, 2} <= set(S.S8) and 1 in S.S32


def test_the_comb_has_one_row_above_the_long_row_threshold():
    N, rp, ci = S.comb(S.N_PATH)
    deg = np.diff(rp)
    assert N == S.N_PATH + S.HUB + 1 and deg[N - 1] == S.HUB + 1 > 4096 and deg[:N - 1].max() == 1
    assert ci[rp[N - 1]] == S.N_PATH - 1 and (np.sort(ci[rp[N - 1] + 1:]) == np.arange(S.N_PATH, N - 1)).all()
    assert (ci[:S.N_PATH - 1] == np.arange(S.N_PATH - 1)).all() and deg[0] == 0 and (deg[S.N_PATH:N - 1] == 0).all()


@pytest.mark.parametrize("sr", SEMIRINGS, ids=S.SR_NAME.get)
def test_every_launch_count_of_S8_is_hit_exactly(sr):
    for L in S.S8:
        x, it, conv = S.iterate_ref(sr, L)
        assert (it, conv) == (L, True), (S.SR_NAME[sr], L, it, conv)
        for cap in S.caps_for(L):
            xc, itc, convc = S.iterate_ref(sr, L, cap)
            assert (itc, convc) == (min(cap, L), cap >= L), (S.SR_NAME[sr], L, cap)
            # (the confirming launch changes nothing: the run cut one launch short holds the final vector, unconfirmed)
            assert np.array_equal(S.bits_of(xc), S.bits_of(x))
            assert np.array_equal(S.bits_of(xc), S.bits_of(S.iterates(sr, L, L)[min(cap, L)]))
        if L > 2:   # ... and every launch before it changes something
            xs = S.iterates(sr, L, L)
            assert all(not np.array_equal(S.bits_of(xs[k]), S.bits_of(xs[k + 1])) for k in range(L - 1))
        c = S.iterate_case(sr, L)
        assert np.diff(c["rp"]).max() == S.HUB + 1
        if sr == S.MM and L > 1:   # the hub's word is still changing in the last launch before the confirming one
            xs = S.iterates(sr, L, L)
            assert xs[L - 1][-1] != xs[L - 2][-1]


@pytest.mark.parametrize("sr", (S.OA, S.MM), ids=S.SR_NAME.get)
def test_the_oracle_and_the_numpy_reference_agree_on_the_integer_combs(sr):
    for L in (1, 2, 8, 9, 25):
        c = S.iterate_case(sr, L)
        for cap in S.caps_for(L) + [S.UNCAPPED]:
            x, it, conv = I.iterate(sr, c["rp"], c["ci"], c["va"], c["x0"], c["x0"], c["alpha"], c["beta"], cap)
            want = S.iterate_ref(sr, L, cap)
            assert (it, conv) == want[1:] and np.array_equal(x, want[0])


def test_the_min_plus_comb_agrees_with_the_order_free_reference():
    for L in (1, 8, 17):
        c = S.iterate_case(S.MP, L)
        x = c["x0"]
        for _ in range(L):
            x = M.order_free(c["rp"], c["ci"], c["va"], x, x, 0.0, 0.0, c["N"])
        assert np.array_equal(M.bits(x), M.bits(S.iterate_ref(S.MP, L)[0]))


def test_the_columns_of_a_multi_source_run_land_in_three_batches():
    for counts in S.COUNTS4:
        assert counts[0] == 1 and len(counts) == 4
    hit = {c for counts in S.COUNTS4 for c in counts}
    assert {1, 8, 9, 16, 17} <= hit
    assert set(S.COUNTS32) == set(S.S8) and S.COUNTS32[0] == 1 and len(S.COUNTS32) == 32
    for counts in S.COUNTS4 + (S.COUNTS32,):
        batches = {(c - 1) // 8 for c in counts}
        assert {0, 1} <= batches and (2 in batches or counts == S.COUNTS4[0])
    for words in (1, 8):
        counts = S.counts_of_sources(32 * words)
        for w in range(words):   # the sources of every count are spread over every word
            assert set(counts[32 * w:32 * w + 32]) == set(S.S8)
    for sr in (S.OA, S.MP):
        for L in S.S8:
            assert S.source_ref(sr, L)[1:] == (L, True)
            assert S.source_for(sr, L) == (S.N_PATH + S.HUB if L == 1 else S.N_PATH + 1 - L)
    assert S.multi_caps(S.COUNTS4[0]) == [1, 7, 8, 9, 15, 16]
    assert S.multi_caps(S.S8) == [1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 23, 24, 25]


def test_the_level_sizes_of_a_comb_source():
    for L in S.S8:
        sizes = S.level_sizes(L, L)
        assert sizes == (1,) * (L - 1) + (0,)     # one new vertex per launch, none in the confirming one


def test_the_frontier_modes_of_the_comb():
    """A launch of the comb changes one row, whose transposed column holds one entry: under every share but 0 all
    launches from 2 on are sparse, so the first batch is cut after launch 1 and the seams move to 2, 10, 18, 26."""
    nnz = len(S.comb(S.N_PATH)[2])
    assert int(0.02 * nnz) >= 2
    for sr in (S.OA, S.MP):
        for L in S.S8:
            assert S.frontier_modes(sr, L, L, 0.0) == [0] * L
            for share in (0.02, 1.0):
                assert S.frontier_modes(sr, L, L, share) == [0, 0][:L] + [1] * max(L - 2, 0)
            assert S.frontier_changed(sr, L, L) == [1] * (L - 1) + [0]


def test_the_directed_path_takes_n_bfs_steps():
    for L in S.S32:
        b = S.bfs_ref(L)
        assert (b.steps, b.depth, b.complete, b.reached) == (L, L - 1, True, L)
        for cap in S.round_caps(L):
            c = S.bfs_ref(L, cap)
            assert (c.steps, c.complete) == (min(cap, L), cap >= L)


def test_the_undirected_path_takes_half_its_length_in_core_rounds():
    for R in S.S32:
        w = S.core_peel(R)
        assert (w["rounds"], w["complete"], w["levels"]) == (R, True, 1) and S.core_path(R)[0] == 2 * R
        for cap in S.round_caps(R):
            c = S.core_peel(R, cap)
            assert (c["rounds"], c["complete"]) == (min(cap, R), cap >= R)
            assert ((c["core"] < 0).any()) == (cap < R)


def test_the_cliques_take_one_truss_round_each():
    for R in S.S32_TRUSS:
        w = S.truss_peel(R)
        assert (w["rounds"], w["levels"], w["complete"], w["max_truss"]) == (R, R, True, R + 2)
        assert w["k"].tolist() == list(range(3, R + 3))
        if R > 1:
            c = S.truss_peel(R, R - 1)
            assert (c["rounds"], c["complete"]) == (R - 1, False) and (c["truss"] == 0).any()
    assert S.truss_cliques(57)[2].size // 2 < 35_000
    full = S.truss_peel(9)
    for cap in (9, 10):   # a cap the run does not reach changes nothing in the reference's answer
        w = S.truss_peel(9, cap)
        assert all(np.array_equal(w[f], full[f]) for f in full), cap


def test_the_inputs_of_the_invariant_tier():
    n, rp, ci, va, x0 = S.sssp_path()
    dist, launches = sssp_ref.fixed_point(rp, ci, va, x0)
    assert launches == n - 1 >= max(S.S32) + 1 and np.array_equal(dist, np.arange(n, dtype=np.float32))
    assert np.array_equal(S.sssp_want()[0], dist) and S.sssp_want()[2] == n
    n, rp, ci, va = S.scc_path()
    _, kinds, sizes = scc_ref.schedule(n, rp, ci, va, 0, 0)
    assert kinds == [2] * 40 and sizes == [1] * 40 and 4 * 40 > max(S.S32)
    assert np.array_equal(S.scc_want(), np.arange(n))
    n, rp, ci, va = S.wcc_grid()
    assert np.diff(rp).max() == 4 < min(S.WCC_SAMPLES) and (S.wcc_want() == n - 1).all()
    for seam in (8, 24):   # rounds > sample: the sampling rounds alone end before, on and behind both seams
        assert {seam - 1, seam} <= set(S.WCC_SAMPLES)
    assert O.OR_AND_I32 == S.OA
