"""The shapes of tests/graph_hygiene_shapes.py make the errors visible that tests/test_graph_hygiene_gpu.py is there to
catch: asserted on the references alone, no engine.

(a) the first and the last element of every expected output vector differ from 0xDEADBEEF, the prefill: an element the
    call left unwritten at either end shows;
(b) per entry point, in one shape at least, the last element is not what the call's own initialisation leaves (level and
    pred -1, dist FLT_MAX or 0, tri 0, core 0, truss 2, support 0, comp[v] = v, color -1 or 0, mate -1, in_msf and
    in_match 0, perm and pos -1): a kernel that stops one element short after a correct initialisation shows.  comp is
    looked at in its first element: the last vertex is the largest of its component whatever the graph.  Every shape has an
    unmatched vertex, a tree edge and an edge outside the forest;
(c) every BFS and SSSP case on a union is two levels deep at least and leaves a vertex unreached, and turning an unreached
    vertex into a source changes the answer: a guard word read as a source shows.  The wheel is connected, so it has no
    unreached vertex; from a rim vertex it is two levels deep, from the hub one level by construction (every vertex is the
    hub's neighbour) -- that case is there for the hub's own element, the last word before the guard;
(d) every shape has a triangle and an edge of truss number >= 3;
(e) rows and M leave the boundaries: the residues modulo 32, 64 and 256 are the ones the shapes were chosen for."""
import numpy as np
import pytest

import graph_hygiene_shapes as S
import small_graphs_ref as R

DEAD32 = np.uint32(S.DEAD)


def outputs(s):
    """(entry point, name, vector) of every expected output vector of a shape."""
    for st in s.starts:
        for name in ("level", "parent"):
            yield "bfs", name, st.bfs[name]
        for name in ("dist", "pred"):
            yield "sssp", name, st.sssp[name]
    for what, names in (("scc", ("comp",)), ("wcc", ("comp",)), ("tri", ("tri", "deg")), ("core", ("core", "deg")),
                        ("truss", ("truss", "support", "edge_u", "edge_v"))):
        for name in names:
            yield what, name, s.want[what][name]
    for name in ("in_msf", "comp", "edge_u", "edge_v", "weight"):
        yield "msf", name, s.want["msf"][name]
    for what, names in (("color", ("color",)), ("match", ("mate", "in_match", "edge_u", "edge_v", "weight")), ("rcm", ("perm", "pos", "level"))):
        for setting, want in s.want[what].items():
            for name in names:
                yield what, name, want[name]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", S.NAMES)
def test_a_word_left_unwritten_at_either_end_shows(name):   # (a)
    s = S.shape(name)
    for what, vec_name, vec in outputs(s):
        want_len = {"tri": s.rows, "truss": s.M, "support": s.M, "edge_u": s.M, "edge_v": s.M}.get(vec_name, s.rows)
        if what in ("msf", "match") and vec_name not in ("comp", "mate"):
            want_len = s.Mw   # the edges of the weighted graph: a stored +0.0 is no entry
        assert len(vec) == want_len > 0, (what, vec_name, len(vec))
        w = words(vec)   # (a uint64 count is two words)
        assert w[0] != DEAD32 and w[-1] != DEAD32 and (vec.dtype != np.uint64 or (w[1] != DEAD32 and w[-2] != DEAD32)), (what, vec_name)


def test_the_last_element_is_not_what_an_initialisation_leaves():   # (b)
    seen = set()
    for name in S.NAMES:
        s = S.shape(name)
        for st in s.starts:
            dist_last = st.sssp["dist"].view(np.float32)[-1]
            seen |= {k for k, ok in (("level", st.bfs["level"][-1] >= 1), ("parent", st.bfs["parent"][-1] != -1),
                                     ("dist", 0 < dist_last < S.FLT_MAX), ("pred", st.sssp["pred"][-1] != -1)) if ok}
        w = s.want
        seen |= {k for k, ok in (("tri", w["tri"]["tri"][-1] > 0), ("core", w["core"]["core"][-1] >= 1),
                                 ("truss", w["truss"]["truss"][-1] >= 3), ("support", w["truss"]["support"][-1] >= 1),
                                 ("scc", w["scc"]["comp"][0] != 0), ("wcc", w["wcc"]["comp"][0] != 0)) if ok}
        seen |= {k for k, ok in (("in_msf", w["msf"]["in_msf"][-1] != 0), ("msf comp", w["msf"]["comp"][0] != 0)) if ok}
        for want in w["color"].values():
            seen |= {"color"} if want["color"][-1] >= 1 else set()
        for want in w["match"].values():
            seen |= {k for k, ok in (("mate", want["mate"][-1] != -1), ("in_match", want["in_match"][-1] != 0)) if ok}
            assert (want["mate"] == -1).any(), (name, "no unmatched vertex")
        for want in w["rcm"].values():
            seen |= {k for k in ("perm", "pos") if want[k][-1] != -1}
        assert (w["msf"]["in_msf"] == 1).any() and (w["msf"]["in_msf"] == 0).any(), (name, "a tree edge and an edge outside the forest")
    assert seen == {"level", "parent", "dist", "pred", "tri", "core", "truss", "support", "scc", "wcc", "in_msf", "msf comp", "color",
                    "mate", "in_match", "perm", "pos"}, seen
    # the wheel alone has them all: the hub's element is the last word before the guard, the hub's edge the last edge id
    s = S.shape("wheel")
    rim = s.starts[0]
    assert rim.bfs["level"][-1] == 1 and rim.bfs["parent"][-1] == S.WHEEL_RIM_SOURCE == rim.sssp["pred"][-1]
    assert rim.sssp["dist"].view(np.float32)[-1] == 0.5
    assert s.want["tri"]["tri"][-1] == S.WHEEL_N - 1 and s.want["core"]["core"][-1] == 3 and s.want["truss"]["truss"][-1] == 3
    assert s.want["truss"]["support"][-1] == 2 and (s.want["truss"]["edge_u"][-1], s.want["truss"]["edge_v"][-1]) == (S.WHEEL_N - 2, S.WHEEL_N - 1)
    assert (s.want["scc"]["comp"] == S.WHEEL_N - 1).all() and (s.want["wcc"]["comp"] == S.WHEEL_N - 1).all()
    # the hub is joined to a cycle, which takes two colours at least: coloured last (order 0: the largest index; prio:
    # the smallest priority) its colour is >= 2.  Every spoke (0.5) is lighter than every rim edge (1): the forest is the
    # spokes, the last edge id among them.  Lightest first by edge id, the first spoke 0 - hub is matched: mate[hub] = 0.
    hub = S.WHEEL_N - 1
    assert s.want["color"][(0, 0, False)]["color"][hub] >= 2 and s.want["color"][(1, 1, True)]["color"][hub] >= 2
    assert s.want["color"][(2, 1, False)]["color"][hub] == 0 and s.prio[hub] == s.prio.min() == -1
    f = s.want["msf"]
    assert f["in_msf"][-1] == 1 and np.array_equal(f["in_msf"] == 1, f["edge_v"] == hub) and (f["comp"] == hub).all()
    assert f["tree_edges"] == S.WHEEL_N - 1 and f["components"] == 1 and (f["edge_u"][-1], f["edge_v"][-1]) == (hub - 1, hub)
    assert s.want["match"][(0, 0)]["mate"][hub] == 0 and s.want["match"][(0, 0)]["mate"][0] == hub
    for setting, want in s.want["match"].items():
        assert (want["mate"] == -1).sum() % 2 == 1   # 4131 vertices: one at least stays alone
    for want in s.want["rcm"].values():
        assert sorted(want["perm"].tolist()) == list(range(S.WHEEL_N)) and want["complete"] and want["components"] == 1
    # a run cut short (one round, one step) has something left to do, and says so in the vectors
    cut = s.cut
    assert all(not c["complete"] and (c["color"] == -1).any() and (c["color"] >= 0).any() for c in cut["color"].values())
    assert not cut["msf"]["complete"] and (cut["msf"]["comp"] == -1).all() and cut["msf"]["in_msf"].any()
    assert all(not m["complete"] and m["pairs"] >= 1 and m["pairs"] < s.want["match"][k]["pairs"] for k, m in cut["match"].items())
    assert all(not r["complete"] and r["steps"] == 1 and (r["perm"] == -1).any() and r["bandwidth_after"] == -1 for r in cut["rcm"].values())


@pytest.mark.parametrize("name", S.UNION_NAMES)
def test_a_guard_word_read_as_a_source_shows_on_a_union(name):   # (c)
    s = S.shape(name)
    (st,) = s.starts
    G, n = s.A.shape[:2]
    assert st.bfs["depth"] >= 2 and (st.bfs["level"] == -1).any() and st.bfs["reached"] < s.rows
    dist = st.sssp["dist"].view(np.float32)
    assert (dist == S.FLT_MAX).any() and st.sssp["reached"] < s.rows
    assert (st.sssp["pred"][st.sssp["pred"] >= 0] != st.sssp["pred"][st.sssp["pred"] >= 0][0]).any()
    pred_local = R.sssp(s.A, s.local["val"], s.local["x0"])["pred"]
    assert ((pred_local >= 0) & (np.take_along_axis(pred_local, np.maximum(pred_local, 0), axis=1) >= 0)).any(), "no SSSP path of two edges"
    # one unreached vertex (the last in the union's order) turned into a source
    local_level = R.gather(st.bfs["level"], G, n, s.numbering)
    g, v = np.argwhere(local_level == -1)[-1]
    src = s.local["src"].copy()
    src[g, v] = True
    b = R.bfs(s.A, src)
    assert b["reached"] > st.bfs["reached"] and b["sizes"][0] == st.bfs["sizes"][0] + 1 and b["level"][g, v] == 0
    x0 = s.local["x0"].copy()
    assert x0[g, v] == S.FLT_MAX and R.gather(dist, G, n, s.numbering)[g, v] == S.FLT_MAX   # the same vertex is unreached under sssp
    x0[g, v] = np.uint32(S.SSSP_X0_GUARD).view(np.float32)
    d = R.sssp(s.A, s.local["val"], x0)
    assert d["reached"] > st.sssp["reached"] and d["dist"][g, v] == 0


def test_the_wheel_is_two_levels_deep_from_the_rim():   # (c), the wheel
    s = S.shape("wheel")
    rim, hub = s.starts
    assert (rim.label, hub.label) == ("rim", "hub")
    assert rim.bfs["depth"] == 2 and rim.bfs["sizes"] == [1, 3, S.WHEEL_N - 4, 0] and rim.bfs["reached"] == S.WHEEL_N
    assert hub.bfs["depth"] == 1 and hub.bfs["sizes"] == [1, S.WHEEL_N - 1, 0] and hub.sources[-1] == 1 and hub.x0[-1] == 0
    assert rim.bfs_cut["complete"] is False and rim.bfs_cut["reached"] == 4 and (rim.bfs_cut["level"] == -1).sum() == S.WHEEL_N - 4
    assert hub.bfs_cut["complete"] is False and hub.bfs_cut["reached"] == S.WHEEL_N
    # rim: 0.5 to the hub, 1 to everybody else (along the rim or over the hub: a tie, the smaller predecessor wins)
    dist = rim.sssp["dist"].view(np.float32)
    assert set(dist.tolist()) == {0.0, 0.5, 1.0} and (dist == 1.0).sum() == S.WHEEL_N - 2
    assert set(rim.sssp["pred"].tolist()) == {-1, S.WHEEL_RIM_SOURCE, S.WHEEL_N - 1}
    assert (hub.sssp["dist"].view(np.float32)[:-1] == 0.5).all() and (hub.sssp["pred"][:-1] == S.WHEEL_N - 1).all()
    # the hub's list is longer than every piece length (2048, 4096) of the handles
    assert np.diff(s.rp).max() == np.diff(s.rp1).max() == S.WHEEL_N - 1 > 4096 and len(s.ci) == 2 * S.WHEEL_M and len(s.ci1) == S.WHEEL_M


@pytest.mark.parametrize("name", S.NAMES)
def test_every_shape_has_a_triangle_and_a_truss_of_three(name):   # (d)
    w = S.shape(name).want
    assert w["tri"]["triangles"] >= 1 and w["truss"]["triangles"] == w["tri"]["triangles"] and w["truss"]["max_truss"] >= 3
    assert (w["truss"]["truss"] >= 3).any() and w["core"]["degeneracy"] >= 2 and (w["tri"]["tri"] > 0).any()
    assert w["truss"]["edges"] == len(w["truss"]["truss"]) == S.shape(name).M


def test_rows_and_edges_leave_every_boundary():   # (e)
    for window, (rows, r32, r64, r256) in S.RESIDUES.items():
        for numbering in R.NUMBERINGS:
            s = S.shape(f"{window}-{numbering}")
            assert (s.rows, s.rows % 32, s.rows % 64, s.rows % 256) == (rows, r32, r64, r256), window
    assert [S.RESIDUES[w][0] % 64 for w in ("u5x13", "u5x19", "u5x45", "u5x51", "u5x1023")] == [1, 31, 33, 63, 59]
    assert S.RESIDUES["u5x1023"][0] % 256 == 251 and S.RESIDUES["d3x181"][0] % 32 != 0
    s = S.shape("wheel")
    assert (s.rows, s.rows % 32, s.rows % 64, s.rows - 1 > 4096) == (4131, 3, 35, True)
    assert (s.M, s.M % 32, s.M % 64, s.M % 256) == (8260, 4, 4, 68)


@pytest.mark.parametrize("name", S.FRONTIER_NAMES)
def test_the_frontier_cases_reach_a_sparse_launch_and_move_the_last_word(name):
    """Launches 0 and 1 are always dense: a run of three launches at least has one that dense_share = 1 makes sparse."""
    for sr in S.FRONTIER_SEMIRINGS:
        va, x0, want, launches, converged = S.frontier_case(name, sr)
        assert converged and 3 <= launches < S.FRONTIER_CAP, (name, sr, launches)
        assert (words(want) != words(x0)).any() and words(want)[0] != DEAD32 and words(want)[-1] != DEAD32
    for sr in S.FRONTIER_SEMIRINGS:   # on the wheel the hub's word, the last before the guard, is one that moves
        va, x0, want, _, _ = S.frontier_case("wheel", sr)
        assert words(want)[-1] != words(x0)[-1]
