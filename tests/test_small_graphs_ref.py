"""tests/small_graphs_ref.py on the CPU: its references against the ones the project already has (scc_ref, wcc_ref,
oracle_bfs, sssp_ref on the union of all 65 536 digraphs on 4 vertices; tri_ref, core_ref, truss_ref on the union of all
32 768 graphs on 6 vertices) and against scipy.sparse.csgraph on the 3-vertex digraphs; that the unions are what they
claim; that they tell a wrong tie-break from a right one (the discrimination counts of DESIGN.md 4, "Exhaustive small
graphs"); and that the two numberings give the same local answers.  The references of the four newer entry points:
coloring against color_ref.first_fit (and color_ref.schedule for the records), msf against msf_ref.kruskal on
msf_ref.edges, matching against match_ref.greedy and certify, on every union of the GPU file under both numberings and
every setting it runs, and graph by graph on the digraphs on 3 and 4 and the graphs on 4 and 5 vertices; rcm_ref.levels
against rcm_ref.serial with the step counts the GPU file pays; and each of five rules broken on purpose changes an
output on some union under each numbering.  Every comparison is ==."""
import numpy as np
import pytest

import color_ref
import core_ref
import match_ref
import msf_ref
import rcm_ref
import scc_ref
import small_graphs_ref as R
import sssp_ref
import tri_ref
import truss_ref
import wcc_ref
from bfs_ref import oracle_bfs


class Case:
    """One union under one numbering, as the CSR arrays the older references take."""

    def __init__(self, A, numbering, stored=None):
        self.A, self.numbering = A, numbering
        self.G, self.n = A.shape[:2]
        self.N = self.G * self.n
        self.rp, self.ci, self.loc = R.union(A, numbering, stored)
        self.ones = np.ones(len(self.ci), np.float32)

    def csr(self):
        return self.N, self.rp, self.ci, self.ones

    def local(self, vector):
        """A union vector of union indices (-1 kept) as (G, n) local indices; a label outside its graph fails."""
        got = R.gather(vector, self.G, self.n, self.numbering).astype(np.int64)
        ids = R.vertex_ids(self.G, self.n, self.numbering)
        back = (got - ids[:, :1]) // (1 if self.numbering == "blocks" else self.G)
        ok = got < 0
        inside = (back >= 0) & (back < self.n)
        assert (ok | (inside & (np.take_along_axis(ids, np.clip(back, 0, self.n - 1), axis=1) == got))).all()
        return np.where(ok, -1, back)


_cases = {}


def digraphs(n, numbering="blocks"):
    if ("d", n, numbering) not in _cases:
        _cases[("d", n, numbering)] = Case(R.all_digraphs(n), numbering)
    return _cases[("d", n, numbering)]


def undirected(n, numbering="blocks"):
    """Stored one way: even graphs the upper triangle, odd graphs the lower."""
    if ("u", n, numbering) not in _cases:
        A = R.all_undirected(n)
        _cases[("u", n, numbering)] = Case(A, numbering, R.halves(A))
    return _cases[("u", n, numbering)]


_refs = {}


def ref(what, A):
    key = (what, A.shape)
    if key not in _refs:
        G, n = A.shape[:2]
        if what == "bfs":
            _refs[key] = R.bfs(A, R.sssp_inputs(G, n)[2])
        elif what == "sssp":
            val, x0, _ = R.sssp_inputs(G, n)
            _refs[key] = R.sssp(A, val, x0)
        else:
            _refs[key] = getattr(R, what)(A)
    return _refs[key]


def sssp_arrays(case):
    """(val per entry, x0 of the union) of a digraph case."""
    val, x0, _ = R.sssp_inputs(case.G, case.n)
    g, r, c = case.loc
    return np.ascontiguousarray(val[g, r, c]), R.scatter(x0, case.numbering)


# ------------------------------------------------------------------ 1. the inputs are what they claim
def test_the_digraph_union_is_what_it_claims():
    d = digraphs(4)
    assert (d.G, d.N, len(d.ci)) == (65_536, 262_144, 524_288)
    assert len(np.unique(d.A.reshape(d.G, -1), axis=0)) == d.G   # every labelled digraph once
    g = 0b1000_0100_0010_0001   # bits 0, 5, 10, 15: the four self-loops and nothing else
    assert np.array_equal(d.A[g], np.eye(4, dtype=bool))
    assert np.array_equal(d.A[1 << 1], np.arange(16).reshape(4, 4) == 1)   # bit 1 is (r, c) = (0, 1)
    scc, wcc = ref("scc", d.A), ref("wcc", d.A)
    assert int((scc == np.arange(4)).sum()) == 135_136 and int((wcc == np.arange(4)).sum()) == 70_048
    b = ref("bfs", d.A)
    assert b["depth"] == 3 and b["sizes"][0] == d.G + (d.G + 2) // 3 and b["sizes"][-1] == 0
    assert sum(b["sizes"]) == b["reached"]
    # the union keeps every graph to itself and every row in local order
    g, r, c = d.loc
    rows = np.repeat(np.arange(d.N), np.diff(d.rp))
    assert np.array_equal(rows, g * 4 + r) and np.array_equal(d.ci, g * 4 + c)
    assert (np.diff(d.ci)[np.diff(rows) == 0] > 0).all()


def test_the_undirected_union_is_what_it_claims():
    u = undirected(6)
    assert (u.G, u.N, len(u.ci)) == (32_768, 196_608, 245_760)   # stored one way: an entry per edge
    assert np.array_equal(u.A, u.A.transpose(0, 2, 1)) and not u.A[:, np.arange(6), np.arange(6)].any()
    g, r, c = u.loc
    assert ((r < c) == (g % 2 == 0)).all()   # even graphs the upper triangle, odd graphs the lower
    t = R.truss(u.A, "blocks")
    assert t["M"] == 245_760 and t["max_truss"] == 6 and t["triangles"] == 81_920
    assert ref("core", u.A)["degeneracy"] == 5
    assert ref("triangles", u.A)["total"] == 81_920
    full = R.union(u.A, "blocks")
    assert len(full[1]) == 2 * 245_760


def test_the_sssp_inputs_are_what_they_claim():
    for n in (3, 4, 5, 6):
        table = R.TABLE[:n, :n]
        off = ~np.eye(n, dtype=bool)
        assert (table[~off] == 0).any() and (table[off] == 0).any()
        assert (table == R.T).any() and R.SMALLEST_WEIGHT == table[table > 0].min()
    assert np.float32(0.5) + R.T == np.float32(0.5)   # below half an ulp of the distances it meets
    val, x0, src = R.sssp_inputs(65_536, 4)
    assert (np.signbit(val[::5]).all() and not np.signbit(val[1:5]).any())   # every fifth graph negated, -0.0 included
    assert (src.sum(axis=1) == np.where(np.arange(65_536) % 3 == 0, 2, 1)).all()
    assert ((np.abs(x0) == R.SECOND_START).sum(axis=1) == (np.arange(65_536) % 3 == 0)).all() and (x0 < 0).any()
    s = ref("sssp", digraphs(4).A)
    own = int((s["pred"] == np.arange(4)).sum())
    print(f"sssp on the 4-vertex digraphs: {s['sweeps']} sweeps, {s['reached']} reached, {own} their own predecessor")
    assert s["sweeps"] > 0 and s["reached"] > 0 and own > 0
    assert s["reached"] == ref("bfs", digraphs(4).A)["reached"]   # the same sources, and every weight is finite


# ------------------------------------------------------------------ 2. against the references the project already has
@pytest.mark.parametrize("numbering", R.NUMBERINGS)
def test_digraph_references_equal_the_projects(numbering):
    """Under "strided" this is also the statement that the numbering changes no local answer: the older references
    work on the union as one graph and know nothing of its parts."""
    d = digraphs(4, numbering)
    assert np.array_equal(scc_ref.components(*d.csr()), R.to_global(ref("scc", d.A), numbering))
    assert np.array_equal(wcc_ref.components(*d.csr()), R.to_global(ref("wcc", d.A), numbering))
    # BFS
    b = ref("bfs", d.A)
    src = R.sssp_inputs(d.G, d.n)[2]
    o = oracle_bfs(d.N, d.rp, d.ci, d.ones, R.scatter(src.astype(np.int32), numbering))
    assert np.array_equal(o.level, R.scatter(b["level"], numbering))
    assert np.array_equal(o.parent, R.to_global(b["parent"], numbering))
    assert (o.depth, o.reached, o.complete, o.sizes, o.m) == (b["depth"], b["reached"], True, b["sizes"], b["edges"] + [0])
    # SSSP: the bits of dist, and pred
    s = ref("sssp", d.A)
    va, x0 = sssp_arrays(d)
    dist, pred, reached, outdeg = sssp_ref.sssp(d.rp, d.ci, va, x0)
    assert np.array_equal(R.bits(dist), R.bits(R.scatter(s["dist"], numbering)))
    assert np.array_equal(pred, R.to_global(s["pred"], numbering))
    assert (reached, outdeg) == (s["reached"], s["out_degrees_of_reached"])
    # and the local answers read back from the older references are the same under either numbering
    assert np.array_equal(d.local(pred), s["pred"]) and np.array_equal(d.local(o.parent), b["parent"])


@pytest.mark.parametrize("numbering", R.NUMBERINGS)
def test_undirected_references_equal_the_projects(numbering):
    u = undirected(6, numbering)
    t = ref("triangles", u.A)
    tri, deg, m = tri_ref.counts(*u.csr())
    assert np.array_equal(tri, R.scatter(t["tri"], numbering).astype(np.uint64))
    assert np.array_equal(deg, R.scatter(t["deg"], numbering)) and m == len(u.ci)
    c = core_ref.peel(*u.csr())
    assert np.array_equal(c["core"], R.scatter(ref("core", u.A)["core"], numbering))
    assert c["degeneracy"] == ref("core", u.A)["degeneracy"]
    k = R.truss(u.A, numbering)
    eu, ev = tri_ref.pairs_of(*u.csr())
    assert np.array_equal(eu, k["edge_u"]) and np.array_equal(ev, k["edge_v"])
    assert np.array_equal(truss_ref.serial(*u.csr()), k["truss"])
    # one answer per local edge, whatever the numbering
    blocks = R.truss(u.A, "blocks")
    key = lambda x: np.lexsort((x["lv"], x["lu"], x["graph"]))   # noqa: E731
    for name in ("truss", "support"):
        assert np.array_equal(k[name][key(k)], blocks[name][key(blocks)])


def test_direction_and_loops_do_not_matter_to_the_simple_graph():
    """The digraph union through tri / core / truss: the references work on the symmetrised, loop-free pattern; the
    older ones get the entries as stored (almost every edge twice, and the loops)."""
    d = digraphs(4)
    t = ref("triangles", d.A)
    tri, deg, m = tri_ref.counts(*d.csr())
    assert np.array_equal(tri, R.scatter(t["tri"], "blocks").astype(np.uint64)) and np.array_equal(deg, R.scatter(t["deg"], "blocks"))
    assert np.array_equal(core_ref.peel(*d.csr())["core"], R.scatter(ref("core", d.A)["core"], "blocks"))
    k = R.truss(d.A, "blocks")
    p = truss_ref.peel(*d.csr())
    assert m == k["M"] == p["M"] and k["M"] < len(d.ci) // 2 + d.G   # fewer edges than entries: pairs stored twice, loops
    for name in ("truss", "support", "edge_u", "edge_v"):
        assert np.array_equal(p[name], k[name]), name
    assert (p["max_truss"], p["triangles"]) == (k["max_truss"], k["triangles"]) == (4, t["total"])
    # and the undirected union through scc / wcc, stored both ways: the two agree there
    A = R.all_undirected(5)
    assert np.array_equal(R.scc(A), R.wcc(A))


def test_against_scipy_on_the_3_vertex_digraphs():
    """So that the definitions are not only our own reading of them."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components, dijkstra
    d = digraphs(3)
    assert (d.G, d.N) == (512, 1536)
    rows = np.repeat(np.arange(d.N), np.diff(d.rp))
    graph = csr_matrix((np.ones(len(d.ci)), (d.ci, rows)), shape=(d.N, d.N))   # entry (c, r): an edge from c to r
    for connection, mine in (("strong", R.scc(d.A)), ("weak", R.wcc(d.A))):
        count, label = connected_components(graph, directed=True, connection=connection)
        top = np.full(count, -1, np.int64)
        np.maximum.at(top, label, np.arange(d.N))
        assert np.array_equal(top[label], R.to_global(mine, "blocks")), connection
    src = R.sssp_inputs(d.G, d.n)[2]
    b = R.bfs(d.A, src)
    dist = dijkstra(graph, directed=True, unweighted=True, indices=np.flatnonzero(R.scatter(src, "blocks"))).min(axis=0)
    assert np.array_equal(np.where(np.isinf(dist), -1, dist).astype(np.int64), R.scatter(b["level"], "blocks"))


# ------------------------------------------------------------------ 3. the unions discriminate
def test_the_unions_tell_a_wrong_tie_break_from_a_right_one():
    """How many vertices (edges) of the unions would get another answer under a rule that is wrong in one way.  The
    figures are recorded in DESIGN.md 4, "Exhaustive small graphs"; each must be > 0 for the GPU file to mean anything."""
    d, u = digraphs(4), undirected(6)
    b, s = ref("bfs", d.A), ref("sssp", d.A)
    k = R.truss(u.A, "blocks")
    counts = dict(
        parent_largest_differs=int((b["parent_largest"] != b["parent"]).sum()),
        pred_largest_differs=int((s["pred_largest"] != s["pred"]).sum()),
        own_pred=int((s["pred"] == np.arange(4)).sum()),
        scc_differs_from_wcc=int((ref("scc", d.A) != ref("wcc", d.A)).sum()),
        truss_differs_from_support_plus_2=int((k["truss"] != k["support"] + 2).sum()))
    # what sssp_preds would give without its bits(dist) != bits(d0) test: a predecessor for a vertex whose start stands
    stands = R.bits(s["dist"]) == R.bits(s["d0"])
    t = s["dist"][:, None, :] + np.abs(R.sssp_inputs(d.G, d.n)[0])
    tied = (d.A & stands[:, :, None] & (R.bits(t) == R.bits(s["dist"])[:, :, None])).any(axis=2)
    counts["start_stands_yet_an_edge_ties"] = int(tied.sum())
    print("discrimination counts:", counts)
    assert all(v > 0 for v in counts.values()), counts
    assert counts == dict(parent_largest_differs=RECORDED[0], pred_largest_differs=RECORDED[1], own_pred=RECORDED[2],
                          scc_differs_from_wcc=RECORDED[3], truss_differs_from_support_plus_2=RECORDED[4],
                          start_stands_yet_an_edge_ties=RECORDED[5])


RECORDED = (15_345, 57_946, 34_647, 80_448, 36_765, 56_994)   # the figures of DESIGN.md, so that a change of the inputs shows


# ------------------------------------------------------------------ 3b. colour, forest, matching, ordering
BY_GRAPH = (("digraphs", 3), ("digraphs", 4), ("undirected", 4), ("undirected", 5))   # the unions of graphs of up to 5 vertices: also graph by graph


def weighted_case(kind, n, numbering, stored_name):
    """-> (A, val (G, n, n), csr = (N, rp, ci, va)): a union with the weights of R.weights as one matrix."""
    key = ("w", kind, n, numbering, stored_name)
    if key not in _cases:
        A = R.graphs_of(kind, n)
        val = R.weights(len(A), n)
        stored = R.storings(kind, A)[stored_name]
        rp, ci, (g, r, c) = R.union(A, numbering, stored)
        _cases[key] = (A if stored is None else A & stored, val, (len(A) * n, rp, ci, np.ascontiguousarray(val[g, r, c])))
    return _cases[key]


def single(A, g, val=None):
    """Graph g alone as CSR arrays (values: ones, or val[g] at the stored positions)."""
    n = A.shape[1]
    r, c = np.nonzero(A[g])
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    va = np.ones(len(c), np.float32) if val is None else np.ascontiguousarray(val[g][r, c])
    return n, rp, c.astype(np.int32), va


def test_the_weights_are_what_they_claim():
    b = R.WBITS
    off = ~np.eye(6, dtype=bool)
    assert (b != b.T)[off].sum() >= 20 and (b == b.T)[off].any()           # asymmetric pairs, and one that is not
    k = R.order_key(b)
    low = np.minimum(k, k.T)[np.triu(off)]
    assert len(np.unique(low)) < len(low)                                   # equal weights on different pairs
    for word in (0xBFC00000, 0x80000000, 0x7F800000, 0x7FC00001):           # -1.5, -0.0, +inf, a NaN
        assert (b[off] == word).any(), hex(word)
    assert (b == 0)[off].sum() == 1 and b[1, 2] == 0 and b[2, 1] != 0       # one stored +0.0, its opposite counts
    assert np.isnan(b.view(np.float32)[1, 5]) and np.isposinf(b.view(np.float32)[0, 4])
    # k is the header's order: -NaN < -inf < -1.5 < -0.0 < +0.0 < 0.5 < +inf < +NaN
    line = np.array([0xFFC00001, 0xFF800000, 0xBFC00000, 0x80000000, 0, 0x3F000000, 0x7F800000, 0x7FC00001], np.uint32)
    assert (np.diff(R.order_key(line).astype(np.int64)) > 0).all()
    for n in (3, 4, 5, 6):   # every special value reaches every size in some graph, bit for bit; every fifth graph negated
        val = R.bits(R.weights(30, n)).reshape(30, n, n)
        for word in (0, 0x80000000, 0xBFC00000, 0x3FC00000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00001):
            assert (val[:, ~np.eye(n, dtype=bool)] == word).any(), (n, hex(word))
        assert np.array_equal(val[0], b[:n, :n] ^ np.uint32(0x80000000)) and np.array_equal(val[1], np.roll(b, -1, (0, 1))[:n, :n])
    assert np.array_equal(R.mix32(np.arange(1000) ^ 7).astype(np.uint32), color_ref.mix32(np.arange(1000) ^ 7))
    assert np.array_equal(R.order_key(b), msf_ref.order_key(b))


@pytest.mark.parametrize("numbering", R.NUMBERINGS)
@pytest.mark.parametrize("kind,n", R.UNIONS, ids=lambda v: str(v))
def test_colouring_equals_the_serial_first_fit(kind, n, numbering):
    """Every setting the GPU file runs, the union as one matrix through color_ref.first_fit; the records the GPU file takes
    from the chain depths (R.color_schedule) against color_ref.schedule, on every union at every setting; on the unions
    of graphs of up to 5 vertices (BY_GRAPH) graph by graph as well, each graph a matrix of its own, under both
    numberings and the settings whose tie does not need the union's index (order 0, with and without prio)."""
    c = digraphs(n, numbering) if kind == "digraphs" else undirected(n, numbering)
    A = c.A
    prio = R.prio_of(c.G, n)
    for order, seed, with_prio in R.COLOR_SETTINGS + ((0, 0, True),):
        mine = R.coloring(A, R.color_keys(A, numbering, order, seed, prio if with_prio else None))
        pv = R.scatter(prio, numbering) if with_prio else None
        color, colors, depth = color_ref.first_fit(*c.csr(), order=order, seed=seed, prio=pv)
        what = (kind, n, numbering, order, seed, with_prio)
        assert np.array_equal(color, R.scatter(mine["color"], numbering)) and colors == mine["colors"], what
        assert np.array_equal(depth, R.scatter(mine["depth"], numbering)), what
        s = color_ref.schedule(*c.csr(), order=order, seed=seed, prio=pv)
        rounds, sizes, edges = R.color_schedule(A, mine["depth"])
        assert s["complete"] and s["rounds"] == rounds and np.array_equal(s["size"], sizes) and np.array_equal(s["edges"], edges), what
        assert np.array_equal(s["color"], color)
        if (kind, n) in BY_GRAPH:
            if order == 0:
                for g in range(c.G):
                    alone = color_ref.first_fit(*single(A, g), order=0, prio=prio[g] if with_prio else None)
                    assert np.array_equal(alone[0], mine["color"][g]) and np.array_equal(alone[2], mine["depth"][g]), (what, g)


@pytest.mark.parametrize("numbering", R.NUMBERINGS)
@pytest.mark.parametrize("kind,n", R.UNIONS, ids=lambda v: str(v))
def test_forest_and_matching_equal_the_serial_loops(kind, n, numbering):
    """msf_ref.kruskal on msf_ref.edges, match_ref.greedy and certify under every (heavy, seed) of the GPU file, the union
    as one matrix under every storing; graph by graph on the unions of graphs of up to 5 vertices (BY_GRAPH), under both
    numberings (seed 0: the tie by the edge id keeps its local order; mix32 of a union's edge id has no counterpart in a
    graph alone)."""
    A0 = R.graphs_of(kind, n)
    for stored_name in R.storings(kind, A0):
        A, val, csr = weighted_case(kind, n, numbering, stored_name)
        N = csr[0]
        eu, ev, weight, k = msf_ref.edges(*csr)
        f = R.msf(A, val, numbering)
        what = (kind, n, numbering, stored_name)
        assert np.array_equal(eu, f["edge_u"]) and np.array_equal(ev, f["edge_v"]), what
        assert np.array_equal(weight, f["weight"]) and np.array_equal(k, f["k"]), what
        in_msf = msf_ref.kruskal(N, eu, ev, k)
        assert np.array_equal(in_msf, f["in_msf"]), what
        assert np.array_equal(msf_ref.labels(N, eu, ev, in_msf), R.to_global(f["comp"], numbering)), what
        assert np.array_equal(f["comp"], R.wcc(A & (R.bits(val).reshape(val.shape) != 0))), what
        for heavy, seed in R.MATCH_SETTINGS:
            m = R.matching(A, val, numbering, heavy, seed)
            keys = match_ref.mkeys(k, heavy, seed)
            mate, chosen = match_ref.greedy(N, eu, ev, keys)
            assert np.array_equal(mate, R.to_global(m["mate"], numbering)) and np.array_equal(chosen, m["in_match"]), (what, heavy, seed)
            assert match_ref.certify(mate, eu, ev, keys) == "" and m["pairs"] == int((mate > np.arange(N)).sum())
        if (kind, n) in BY_GRAPH:
            zero = {h: R.matching(A, val, numbering, h, 0) for h in (0, 1)}
            by_graph = np.argsort(f["graph"], kind="stable")   # the edges of a graph, in ascending edge id
            start = np.concatenate([[0], np.cumsum(np.bincount(f["graph"], minlength=len(A)))])
            for g in range(len(A)):
                one = single(A, g, val)
                mine = by_graph[start[g]:start[g + 1]]
                eu1, ev1, w1, k1 = msf_ref.edges(*one)
                assert np.array_equal(eu1, f["lu"][mine]) and np.array_equal(ev1, f["lv"][mine]) and np.array_equal(w1, f["weight"][mine]), (what, g)
                assert np.array_equal(msf_ref.kruskal(n, eu1, ev1, k1), f["in_msf"][mine]), (what, g)
                for h in (0, 1):
                    mate, chosen = match_ref.greedy(n, eu1, ev1, match_ref.mkeys(k1, h, 0))
                    assert np.array_equal(mate, zero[h]["mate"][g]) and np.array_equal(chosen, zero[h]["in_match"][mine]), (what, g, h)


def test_the_rcm_step_counts_of_the_unions():
    """sh_rcm has no tensor form: the GPU file takes rcm_ref.levels on the union as one matrix.  Here: it equals the
    serial definition there, and the steps the GPU file pays at sweeps = 8 are the ones it was planned with."""
    steps = {}
    for kind, n in R.RCM_UNIONS:
        c = digraphs(n) if kind == "digraphs" else undirected(n)
        lv, se = rcm_ref.levels(*c.csr(), sweeps=8, reverse=1), rcm_ref.serial(*c.csr(), sweeps=8, reverse=1)
        for f in ("perm", "pos", "level"):
            assert np.array_equal(lv[f], se[f]), (kind, n, f)
        steps[(kind, n)] = (lv["components"], lv["steps"])
        assert lv["steps"] <= 20_000
    assert steps == {("undirected", 4): (98, 579), ("digraphs", 3): (600, 3_672), ("undirected", 5): (1_398, 10_824)}, steps


@pytest.mark.parametrize("numbering", R.NUMBERINGS)
def test_the_unions_tell_a_broken_rule_of_the_four_from_the_right_one(numbering):
    """Each rule broken on purpose changes an output on some union under this numbering (the count of differing
    elements is printed per rule and union)."""
    counts = {}
    for kind, n in R.UNIONS:
        A0 = R.graphs_of(kind, n)
        G = len(A0)
        d = {}
        right = R.coloring(A0, R.color_keys(A0, numbering, 0, 0))["color"]
        d["colour: ties by the larger id"] = int((R.coloring(A0, R.color_keys(A0, numbering, 0, 0, tie="larger"))["color"] != right).sum())
        right = R.coloring(A0, R.color_keys(A0, numbering, 1, 1))["color"]
        d["colour: mix32 of the local id"] = int((R.coloring(A0, R.color_keys(A0, numbering, 1, 1, ids="local"))["color"] != right).sum())
        for stored_name in R.storings(kind, A0):
            A, val, _ = weighted_case(kind, n, numbering, stored_name)
            f = R.msf(A, val, numbering)
            m = {hs: R.matching(A, val, numbering, *hs) for hs in R.MATCH_SETTINGS}

            def differs(a, b, names):
                return int(a["M"] != b["M"]) or sum(int((a[x] != b[x]).sum()) for x in names)
            add = lambda name, v: d.__setitem__(name, d.get(name, 0) + v)   # noqa: E731
            add("forest: ties by the larger id", differs(R.msf(A, val, numbering, tie="larger"), f, ("in_msf",)))
            add("matching: ties by the larger id", differs(R.matching(A, val, numbering, 0, 0, tie="larger"), m[(0, 0)], ("mate",)))
            add("forest: the first entry", differs(R.msf(A, val, numbering, entry="first"), f, ("in_msf", "weight")))
            add("matching: the first entry", differs(R.matching(A, val, numbering, 1, 1, entry="first"), m[(1, 1)], ("mate",)))
            add("forest: +0.0 counted", differs(R.msf(A, val, numbering, zero_counts=True), f, ("in_msf", "comp")))
            add("matching: +0.0 counted", differs(R.matching(A, val, numbering, 1, 1, zero_counts=True), m[(1, 1)], ("mate",)))
            add("matching: heavy ignored", differs(m[(0, 1)], m[(1, 1)], ("mate",)))
            add("matching: mix32 of the local id", differs(R.matching(A, val, numbering, 1, 1, ids="local"), m[(1, 1)], ("mate",)))
        counts[(kind, n)] = d
        print(f"{kind}{n}-{numbering}: {d}")
    for rule in next(iter(counts.values())):
        assert any(d[rule] > 0 for d in counts.values()), (rule, numbering)


# ------------------------------------------------------------------ 4. a failure is told as a small graph
def test_a_mismatch_names_the_smallest_graph():
    d = digraphs(4, "strided")
    want = R.to_global(ref("scc", d.A), "strided")
    assert R.explain_vertices(d.A, "strided", want, want.copy(), True) == ""
    got = want.copy()
    ids = R.vertex_ids(d.G, 4, "strided")
    got[ids[0x0123, 2]] = ids[0x0123, 0]
    got[ids[0x4000, 1]] = 5
    text = R.explain_vertices(d.A, "strided", want, got, True)
    assert "2 of 65536 graphs differ" in text and "g = 291 (0x123), n = 4" in text and "row 0 stores [0, 1]" in text
    assert f"expected per local vertex: {ref('scc', d.A)[0x0123].tolist()}" in text
    u = undirected(6)
    k = R.truss(u.A, "blocks")
    got = k["truss"].copy()
    got[np.flatnonzero(k["graph"] == 77)[1]] += 1
    got[-1] += 1
    text = R.explain_edges(u.A, k, k["truss"], got)
    assert "2 graphs differ" in text and "g = 77 (0x4d), n = 6" in text and "its edges (local ends): ['0-1', '0-3', '0-4', '1-3']" in text


# ------------------------------------------------------------------ 5. one graph checked by eye
def test_the_diamond_drawn_by_hand():
    """0 -> 1, 0 -> 2, 1 -> 3, 2 -> 3 out of the 4-vertex union, the answers written down here and not computed: the
    parent of 3 is 1 (the smaller of two one level up), its predecessor is 2 (the lighter way), and 2, reached over an edge
    of weight 0 from a source at 0, has moved off FLT_MAX and so has a predecessor."""
    g = sum(1 << (4 * r + c) for r, c in ((1, 0), (2, 0), (3, 1), (3, 2)))
    A = R.all_digraphs(4)[g:g + 1]
    val, x0, src = (a[g:g + 1] for a in R.sssp_inputs(65_536, 4))
    assert g == 24_848 and src[0].tolist() == [True, False, False, False] and (val[0] == R.TABLE[:4, :4]).all()
    assert [R.TABLE[r, c] for r, c in ((1, 0), (2, 0), (3, 1), (3, 2))] == [1, 0, 2, 0.5]
    b = R.bfs(A, src)
    assert b["level"][0].tolist() == [0, 1, 1, 2] and b["parent"][0].tolist() == [-1, 0, 0, 1]
    assert b["parent_largest"][0].tolist() == [-1, 0, 0, 2] and b["sizes"] == [1, 2, 1, 0] and b["edges"] == [2, 2, 0]
    s = R.sssp(A, val, x0)
    assert s["dist"][0].tolist() == [0, 1, 0, 0.5] and s["pred"][0].tolist() == [-1, 0, 0, 2]
    assert R.scc(A)[0].tolist() == [0, 1, 2, 3] and R.wcc(A)[0].tolist() == [3, 3, 3, 3]
    t, k = R.triangles(A), R.truss(A, "blocks")
    assert t["tri"][0].tolist() == [0, 0, 0, 0] and t["deg"][0].tolist() == [2, 2, 2, 2] and R.core(A)["core"][0].tolist() == [2] * 4
    assert k["truss"].tolist() == [2] * 4 and list(zip(k["edge_u"].tolist(), k["edge_v"].tolist())) == [(0, 1), (0, 2), (1, 3), (2, 3)]
