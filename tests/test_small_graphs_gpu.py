"""The eleven graph entry points on every small graph at once: the disjoint union of all digraphs with loops on 3 and
on 4 vertices and of all simple graphs on 4, 5 and 6 vertices, each union one matrix, one handle and one call per entry
point, under the two numberings of tests/small_graphs_ref.py (the vertices of a graph in neighbouring lanes / in
different workgroups), against the references written there from the definitions (tests/test_small_graphs_ref.py pins
them on the CPU).  Every union goes through the first seven: the undirected ones, stored both ways, through bfs, sssp,
scc and wcc, where scc == wcc must hold as well; the digraph ones through tri, core and truss, whose graph is the
symmetrised, loop-free pattern -- almost every edge stored twice, and the loops must vanish.  For tri, core, truss and
wcc the undirected unions are stored ONE way (even graphs the upper triangle, odd graphs the lower): direction must not
matter.

color, msf, match and rcm, whose graph is the simple undirected one as well, get the digraph unions as they are and the
undirected unions one way.  msf and match read the values: every entry carries small_graphs_ref.weights -- the two
directions of a pair differ, many pairs tie, and -1.5, -0.0, +inf, a NaN and one stored +0.0 (no entry) are among them
-- and they get the undirected unions stored both ways once more, where the smaller of the two entries decides.  The
ties of color (orders 1 and 2) and match (seed != 0) hash the UNION's vertex or edge id, so under "strided" the order
inside a graph is another one than under "blocks".  color, msf and match are round-parallel (3 to 6 rounds on a union)
and run on all five unions.  sh_rcm takes its steps component by component: a union costs steps, not rounds -- 579
(undirected-4), 3 672 (digraphs-3) and 10 824 (undirected-5) at sweeps = 8, but 368 889 (undirected-6) and 565 488
(digraphs-4), which at the 19 to 29 us per step measured on the grid would be 8 to 12 s per call.  rcm therefore runs on
the first three only, asserts that the reference counts at most 20 000 steps on each, and is interleaved
(test_a_handle_carries_nothing_over) on the unions that have its handle.

Every comparison is == on integer arrays or on uint32 views; there is no tolerance anywhere.  A mismatch is reported as
the smallest failing graph: its bit pattern, n, local adjacency and the local expected and actual rows.
"""
import numpy as np
import pytest

import color_ref
import match_ref
import msf_ref
import rcm_ref
import small_graphs_ref as R
from guarded import _not_halted, call   # noqa: F401  (autouse: after a failed HIP call nothing more is started on the device)
from sparseharness_amd.engine import Engine
from test_rcm_gpu import same as same_as_rcm_gpu      # every scalar and record of a call against rcm_ref.levels
from test_scc_gpu import SETTINGS as SCC_SETTINGS   # the four (trim, pivot) settings

pytestmark = pytest.mark.gpu

UNIONS = R.UNIONS
KEYS = tuple(u + (numbering,) for u in UNIONS for numbering in R.NUMBERINGS)
RCM_KEYS = tuple(u + (numbering,) for u in R.RCM_UNIONS for numbering in R.NUMBERINGS)
ENTRY_POINTS = ("bfs", "sssp", "scc", "wcc", "tri", "core", "truss", "color", "msf", "match", "rcm")
MAX_RCM_STEPS = 20_000
TOP_DOWN, BOTTOM_UP, DEFAULT = (1.0, 0.0), (0.0, 0.0), (-1.0, -1.0)
# bucket widths: below the smallest non-zero weight (every distinct distance a bucket of its own), the default, one bucket
DELTAS = (float(R.SMALLEST_WEIGHT) / 2, -1.0, float("inf"))
SAMPLES = (0, 1, 2, 4)
ORDERS = (0, 1)
CHASES = (0, 4)
# caps no run here comes near (a BFS has at most 6 levels; the rounds are counted in the prints): they only keep the
# per-round arrays of the binding small
MAX_LEVELS, MAX_ROUNDS = 64, 1 << 14
DEFAULTS = dict(color=(2, 0, False), msf=None, match=(1, 1), rcm=(8, 1))   # the settings of the default calls of the newer four


def down(v, dtype, n):
    """v.download through guarded.call."""
    return call(v.download, dtype, n=n)


def key_id(key):
    return f"{key[0]}{key[1]}-{key[2]}"


class Bundle:
    """One union under one numbering: its CSR arrays, the references, and the handles of all eleven entry points (tri
    has one per order, msf and match one per storing, rcm on the unions of R.RCM_UNIONS only), alive together until the
    module is done."""

    def __init__(self, eng, kind, n, numbering):
        self.eng, self.kind, self.n, self.numbering = eng, kind, n, numbering
        self.A = A = R.all_digraphs(n) if kind == "digraphs" else R.all_undirected(n)
        self.G, self.N = len(A), len(A) * n
        self.rp, self.ci, (g, r, c) = R.union(A, numbering)
        ones = np.ones(len(self.ci), np.float32)
        val, x0, src = R.sssp_inputs(self.G, n)
        self.val = np.ascontiguousarray(val[g, r, c])
        self.x0 = R.scatter(x0, numbering)
        self.sources = R.scatter(src.astype(np.int32), numbering)
        # the simple graph's entry points: the digraphs as they are, the undirected graphs stored one way
        one_way = (self.rp, self.ci) if kind == "digraphs" else R.union(A, numbering, R.halves(A))[:2]
        ones_one_way = np.ones(len(one_way[1]), np.float32)
        self.handles = dict(bfs=eng.bfs_graph(self.rp, self.ci, ones), sssp=eng.sssp_graph(self.rp, self.ci, self.val),
                            scc=eng.scc_graph(self.rp, self.ci, ones), wcc=eng.wcc_graph(*one_way, ones_one_way),
                            core=eng.core_graph(*one_way, ones_one_way), truss=eng.truss_graph(*one_way, ones_one_way))
        for order in ORDERS:
            self.handles[("tri", order)] = eng.tri_graph(*one_way, ones_one_way, order=order)
        self.entries, self.entries_one_way = len(self.ci), len(one_way[1])
        # colour and rcm: the pattern as tri, core and truss get it; msf and match: the weights, under every storing.
        # Every device step of the four -- creating a handle, a vector up or down, the call -- goes through guarded.call.
        self.has_rcm = (kind, n) in R.RCM_UNIONS
        self.one_way = (self.N,) + tuple(one_way) + (ones_one_way,)
        self.handles["color"] = call(eng.color_graph, *one_way, ones_one_way)
        if self.has_rcm:
            self.handles["rcm"] = call(eng.rcm_graph, *one_way, ones_one_way)
        self.prio_local = R.prio_of(self.G, n)
        self.prio = R.scatter(self.prio_local, numbering)
        self.wval = R.weights(self.G, n)
        self.weighted = {}
        for storing, mask in R.storings(kind, A).items():
            rp, ci, (wg, wr, wc) = R.union(A, numbering, mask)
            va = np.ascontiguousarray(self.wval[wg, wr, wc])
            self.weighted[storing] = (A if mask is None else A & mask, (self.N, rp, ci, va))
            self.handles[("msf", storing)] = call(eng.msf_graph, rp, ci, va)
            self.handles[("match", storing)] = call(eng.match_graph, rp, ci, va)
        self.storing = next(iter(self.weighted))   # the one the default calls use
        self._refs = {}
        # the references, computed once and never changed
        b, s, t, c_, self.k = R.bfs(A, src), R.sssp(A, val, x0), R.triangles(A), R.core(A), R.truss(A, numbering)
        for d in (b, s, t, c_):
            for a in d.values():
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
        self.want = dict(
            bfs=dict(level=R.scatter(b["level"], numbering).astype(np.int32), parent=R.to_global(b["parent"], numbering).astype(np.int32),
                     depth=b["depth"], reached=b["reached"], complete=True, sizes=b["sizes"]),
            bfs_edges=b["edges"],
            sssp=dict(dist=R.bits(R.scatter(s["dist"], numbering)), pred=R.to_global(s["pred"], numbering).astype(np.int32),
                      reached=s["reached"], complete=True),
            sssp_out_degrees=s["out_degrees_of_reached"],
            scc=dict(comp=R.to_global(R.scc(A), numbering).astype(np.int32)),
            wcc=dict(comp=R.to_global(R.wcc(A), numbering).astype(np.int32)),
            tri=dict(tri=R.scatter(t["tri"], numbering).astype(np.uint64), deg=R.scatter(t["deg"], numbering).astype(np.int32),
                     total=t["total"]),
            core=dict(core=R.scatter(c_["core"], numbering).astype(np.int32), deg=R.scatter(t["deg"], numbering).astype(np.int32),
                      degeneracy=c_["degeneracy"]),
            truss=dict(truss=self.k["truss"], support=self.k["support"], edge_u=self.k["edge_u"], edge_v=self.k["edge_v"],
                       max_truss=self.k["max_truss"], triangles=self.k["triangles"]))
        for name in ("scc", "wcc"):
            comp = self.want[name]["comp"]
            self.want[name]["components"] = int(np.count_nonzero(comp == np.arange(self.N)))

    def free(self):
        for h in self.handles.values():
            h.free()

    # ---- one call of each entry point -> dict of everything that must not depend on the setting
    def vec(self, n, fill=7):
        return self.eng.alloc(max(n, 1)).fill(fill, np.int32)

    def bfs(self, shares=DEFAULT, with_parent=True):
        xv, lv = self.eng.vector(self.sources), self.vec(self.N)
        pv = self.vec(self.N) if with_parent else None
        try:
            depth, reached, complete, modes, sizes, edges, _, _ = self.eng.bfs_levels(
                self.handles["bfs"], xv, lv, pv, max_levels=MAX_LEVELS, up_share=shares[0], down_share=shares[1])
            got = dict(level=lv.download(np.int32, n=self.N), depth=depth, reached=reached, complete=complete, sizes=sizes.tolist())
            if with_parent:
                got["parent"] = pv.download(np.int32, n=self.N)
            assert np.array_equal(xv.download(np.int32, n=self.N), self.sources)   # x0 is only read
            return got, modes.tolist(), edges.tolist()
        finally:
            for v in (xv, lv, pv):
                if v is not None:
                    v.free()

    def sssp(self, delta=-1.0, with_pred=True):
        xv, dv = self.eng.vector(self.x0), self.vec(self.N)
        pv = self.vec(self.N) if with_pred else None
        try:
            rounds, buckets, reached, complete, relaxed, _, _, _, _ = self.eng.sssp(self.handles["sssp"], xv, dv, pv, delta=delta,
                                                                                     max_rounds=MAX_ROUNDS)
            got = dict(dist=dv.download(np.uint32, n=self.N), reached=reached, complete=complete)
            if with_pred:
                got["pred"] = pv.download(np.int32, n=self.N)
            assert np.array_equal(xv.download(np.uint32, n=self.N), R.bits(self.x0))   # x0 is only read
            return got, relaxed, (rounds, buckets)
        finally:
            for v in (xv, dv, pv):
                if v is not None:
                    v.free()

    def scc(self, trim=1, pivot=1):
        cv = self.vec(self.N)
        try:
            res = self.eng.scc(self.handles["scc"], cv, trim=trim, pivot=pivot, max_steps=MAX_ROUNDS)
            assert res[1] == self.N and res[5]   # settled, complete
            return dict(comp=cv.download(np.int32, n=self.N), components=res[0])
        finally:
            cv.free()

    def wcc(self, sample=2):
        cv = self.vec(self.N)
        try:
            res = self.eng.wcc(self.handles["wcc"], cv, sample=sample, max_rounds=MAX_ROUNDS)
            assert res[3]   # complete
            return dict(comp=cv.download(np.int32, n=self.N), components=res[0])
        finally:
            cv.free()

    def tri(self, order=1):
        tv, dv = self.vec(2 * self.N), self.vec(self.N)
        try:
            total, _, _ = self.eng.triangles(self.handles[("tri", order)], tv, dv)
            return dict(tri=tv.download(np.uint32, 2 * self.N).view(np.uint64), deg=dv.download(np.int32, self.N), total=total)
        finally:
            tv.free()
            dv.free()

    def core(self, chase=0):
        cv, dv = self.vec(self.N), self.vec(self.N)
        try:
            res = self.eng.core_numbers(self.handles["core"], cv, dv, chase=chase)
            assert res[3]   # complete
            return dict(core=cv.download(np.int32, self.N), deg=dv.download(np.int32, self.N), degeneracy=res[0])
        finally:
            cv.free()
            dv.free()

    def truss(self):
        m = self.handles["truss"].edges
        vecs = {name: self.vec(m) for name in ("truss", "support", "edge_u", "edge_v")}
        try:
            res = self.eng.truss_numbers(self.handles["truss"], *(vecs[name] for name in ("truss", "support", "edge_u", "edge_v")))
            assert res[3]   # complete
            got = {name: v.download(np.int32, m) if m else np.zeros(0, np.int32) for name, v in vecs.items()}
            got.update(max_truss=res[0], triangles=res[4])
            return got
        finally:
            for v in vecs.values():
                v.free()

    def gvec(self, n, fill=7):
        """vec() for the four newer entry points: a failed HIP call ends the module's GPU work."""
        return call(call(self.eng.alloc, max(n, 1)).fill, fill, np.int32)

    def color(self, setting=(2, 0, False)):
        order, seed, with_prio = setting
        cv = self.gvec(self.N)
        pv = call(self.eng.vector, self.prio) if with_prio else None
        try:
            colors, rounds, complete, coloured, sizes, edges, _, _ = call(
                self.eng.greedy_colors, self.handles["color"], cv, pv, order=order, seed=seed)
            if with_prio:
                assert np.array_equal(down(pv, np.int32, self.N), self.prio)   # prio is only read
            return (dict(color=down(cv, np.int32, self.N), colors=colors, coloured=coloured, complete=complete),
                    (rounds, sizes.tolist(), edges.tolist()))
        finally:
            for v in (cv, pv):
                if v is not None:
                    v.free()

    def msf(self, storing=None, optional=True):
        G = self.handles[("msf", storing or self.storing)]
        m = G.edges
        names = ("in_msf", "comp", "edge_u", "edge_v", "weight") if optional else ("in_msf",)
        vecs = {name: self.gvec(self.N if name == "comp" else m) for name in names}
        try:
            res = call(self.eng.spanning_forest, G, *(vecs.get(name) for name in ("in_msf", "comp", "edge_u", "edge_v", "weight")))
            got = {name: down(v, np.uint32 if name == "weight" else np.int32, self.N if name == "comp" else m)
                   for name, v in vecs.items()}
            got.update(tree_edges=res[0], components=res[1], complete=res[3])
            return got, (res[2], res[4].tolist(), res[5].tolist(), res[6].tolist())
        finally:
            for v in vecs.values():
                v.free()

    def match(self, setting=(1, 1), storing=None, optional=True):
        G = self.handles[("match", storing or self.storing)]
        m = G.edges
        vecs = dict(mate=self.gvec(self.N))
        if optional:
            vecs["in_match"] = self.gvec(m)
        try:
            res = call(self.eng.matching, G, vecs["mate"], heavy=setting[0], seed=setting[1], in_match=vecs.get("in_match"),
                       max_rounds=MAX_ROUNDS)
            got = {name: down(v, np.int32, self.N if name == "mate" else m) for name, v in vecs.items()}
            got.update(pairs=res[0], complete=res[2])
            return got, (res[1], res[3].tolist(), res[4].tolist(), res[5].tolist())
        finally:
            for v in vecs.values():
                v.free()

    def rcm(self, setting=(8, 1)):
        G = self.handles["rcm"]   # (a KeyError on the two large unions: R.RCM_UNIONS)
        vecs = [self.gvec(self.N) for _ in range(3)]
        try:
            res = call(self.eng.rcm_order, G, *vecs, sweeps=setting[0], reverse=setting[1], max_steps=MAX_RCM_STEPS + 1)
            got = dict(zip(("perm", "pos", "level"), (down(v, np.int32, self.N) for v in vecs)))
            got.update(zip(("components", "sweeps_run", "steps", "complete", "bandwidth_before", "bandwidth_after", "profile_before",
                            "profile_after", "kind", "size", "edges"), res[:11]))
            return got, dict(ns=res[11], M=G.edges, max_degree=G.max_degree, footprint=G.footprint)
        finally:
            for v in vecs:
                v.free()

    # ---- the references of the four, each computed once and never changed
    def ref(self, what, setting=None, storing=None):
        """-> (want, records, edge reference): what a call's outputs and its records must equal."""
        storing = storing or self.storing
        key = (what, setting, storing if what in ("msf", "match") else None)
        if key not in self._refs:
            self._refs[key] = getattr(self, "_ref_" + what)(setting, storing)
            for d in self._refs[key][:1] + self._refs[key][2:]:
                for a in (d or {}).values():
                    if isinstance(a, np.ndarray):
                        a.flags.writeable = False
        return self._refs[key]

    def _ref_color(self, setting, storing):
        order, seed, with_prio = setting
        c = R.coloring(self.A, R.color_keys(self.A, self.numbering, order, seed, self.prio_local if with_prio else None))
        rounds, sizes, edges = R.color_schedule(self.A, c["depth"])
        if self.N <= 6_000:   # the model walks vertex by vertex: on the larger unions the CPU file pins this at every setting
            s = color_ref.schedule(*self.one_way, order=order, seed=seed, prio=self.prio if with_prio else None)
            assert (s["rounds"], s["size"].tolist(), s["edges"].tolist()) == (rounds, sizes.tolist(), edges.tolist())
        return (dict(color=R.scatter(c["color"], self.numbering).astype(np.int32), colors=c["colors"], coloured=self.N, complete=True),
                (rounds, sizes.tolist(), edges.tolist()), None)

    def _ref_msf(self, setting, storing):
        A, csr = self.weighted[storing]
        f = R.msf(A, self.wval, self.numbering)
        s = msf_ref.schedule(*csr)
        assert s["complete"] and s["M"] == f["M"]
        return (dict(in_msf=f["in_msf"], comp=R.to_global(f["comp"], self.numbering).astype(np.int32), edge_u=f["edge_u"],
                     edge_v=f["edge_v"], weight=f["weight"], tree_edges=f["tree_edges"], components=f["components"], complete=True),
                (s["rounds"], s["walked"].tolist(), s["kept"].tolist(), s["hooks"].tolist()), f)

    def _ref_match(self, setting, storing):
        A, csr = self.weighted[storing]
        m = R.matching(A, self.wval, self.numbering, *setting)
        eu, ev, _, k = msf_ref.edges(*csr)
        s = match_ref.rounds(self.N, eu, ev, match_ref.mkeys(k, *setting))
        assert s["complete"]
        return (dict(mate=R.to_global(m["mate"], self.numbering).astype(np.int32), in_match=m["in_match"], pairs=m["pairs"], complete=True),
                (s["rounds"], s["walked"].tolist(), s["kept"].tolist(), s["matched"].tolist()), m)

    def _ref_rcm(self, setting, storing):
        w = rcm_ref.levels(*self.one_way, sweeps=setting[0], reverse=setting[1])
        serial = rcm_ref.serial(*self.one_way, sweeps=setting[0], reverse=setting[1])
        assert all(np.array_equal(w[f], serial[f]) for f in ("perm", "pos", "level")) and w["components"] == serial["components"]
        extra = {f: w.pop(f) for f in ("M", "max_degree", "roots", "done")}
        return w, None, extra

    def default_call(self, what):
        """-> the outputs of one call of an entry point at its default setting (what the interleaving test compares)."""
        got = getattr(self, what)()
        assert got is not None, (what, "this union has no handle of it")
        return got[0] if isinstance(got, tuple) else got

    # ---- comparing
    def check(self, what, got, setting, ref=None):
        """Every output of `got` equals the reference's; a vector that differs is told as the smallest failing graph.
        ref: (want, records, edge reference) of Bundle.ref for a call of the newer four that is not the default one."""
        if what in DEFAULTS and ref is None:
            ref = self.ref(what, DEFAULTS[what])
        want, edge_ref = (self.want[what], None) if ref is None else (ref[0], ref[2])
        assert set(got) <= set(want), (set(got), set(want))
        for name, value in got.items():
            expected = want[name]
            if not isinstance(expected, np.ndarray):
                assert value == expected, f"{what} {key_id((self.kind, self.n, self.numbering))} {setting}: {name} {value}, expected {expected}"
                continue
            if np.array_equal(value, expected):
                continue
            if what == "truss":
                if name in ("edge_u", "edge_v") or len(value) != len(expected):
                    text = f"{len(value)} edges, expected {len(expected)}; first difference at edge {int(np.flatnonzero(value != expected)[0]) if len(value) == len(expected) else '?'}"
                else:
                    text = R.explain_edges(self.A, self.k, expected, value)
            elif name in ("in_msf", "in_match", "weight", "edge_u", "edge_v"):   # per edge of the weighted graph
                text = R.explain_edges(self.A, edge_ref, expected, value)
            elif name in ("perm", "kind", "size", "edges"):   # per position, per step
                text = (f"lengths {len(value)}, expected {len(expected)}" if len(value) != len(expected) else
                        f"first difference at {int(np.flatnonzero(value != expected)[0])}")
            else:
                inputs = {}
                if what == "bfs":
                    inputs = {"source": self.sources}
                if what == "sssp":   # (an entry at (r, c) weighs small_graphs_ref.TABLE[r, c] in every graph)
                    inputs = {"x0": self.x0}
                show = (lambda v: v.view(np.float32)) if name == "dist" else None   # compared as bits, shown as floats
                text = R.explain_vertices(self.A, self.numbering, expected, value, name in ("parent", "pred", "comp", "mate"), inputs, show)
            raise AssertionError(f"{what} {key_id((self.kind, self.n, self.numbering))} {setting}: {name} differs\n{text}")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bundles(eng):
    """bundle(key): the union's handles, built at first use and kept alive, all of them, until the module is done."""
    made = {}

    def bundle(key):
        if key not in made:
            made[key] = Bundle(eng, *key)
        return made[key]
    yield bundle
    for b in made.values():
        b.free()


def same(first, again):
    return first.keys() == again.keys() and all(np.array_equal(first[k], again[k]) for k in first)


# ------------------------------------------------------------------ 1. every union through every entry point
@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_bfs_levels_in_every_direction(bundles, key):
    B = bundles(key)
    assert B.handles["bfs"].edges == B.entries
    for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
        got, modes, edges = B.bfs(shares)
        B.check("bfs", got, f"shares {shares}")
        if shares == TOP_DOWN:
            assert modes == [0] * len(modes) and edges == B.want["bfs_edges"], (edges, B.want["bfs_edges"])
        if shares == BOTTOM_UP:
            assert modes == [1] * len(modes)
        without, _, _ = B.bfs(shares, with_parent=False)
        B.check("bfs", without, f"shares {shares}, parent=None")
        assert "parent" not in without and same(without, {k: v for k, v in got.items() if k != "parent"})


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_sssp_under_three_bucket_widths(bundles, key):
    B = bundles(key)
    assert B.handles["sssp"].edges == B.entries   # a stored zero and a stored -0.0 are edges of weight 0
    assert B.handles["sssp"].delta > float(R.SMALLEST_WEIGHT)
    for delta in DELTAS:
        got, relaxed, (rounds, buckets) = B.sssp(delta)
        print(f"{key_id(key)} delta {delta}: rounds {rounds} buckets {buckets} relaxed {relaxed}")
        B.check("sssp", got, f"delta {delta}")
        assert relaxed >= B.want["sssp_out_degrees"], (delta, relaxed)
        without, relaxed, _ = B.sssp(delta, with_pred=False)
        B.check("sssp", without, f"delta {delta}, pred=None")
        assert relaxed >= B.want["sssp_out_degrees"] and "pred" not in without


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_scc_under_every_setting(bundles, key):
    B = bundles(key)
    assert B.handles["scc"].edges == B.entries
    for trim, pivot in SCC_SETTINGS:
        B.check("scc", B.scc(trim, pivot), f"trim {trim} pivot {pivot}")
    if B.kind == "undirected":   # stored both ways: what hangs together does so strongly
        assert np.array_equal(B.want["scc"]["comp"], B.want["wcc"]["comp"])
        assert np.array_equal(B.scc()["comp"], B.wcc()["comp"])


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_wcc_at_every_sample(bundles, key):
    B = bundles(key)
    assert B.handles["wcc"].edges == B.entries_one_way
    for sample in SAMPLES:
        B.check("wcc", B.wcc(sample), f"sample {sample}")


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_triangles_under_both_orders(bundles, key):
    B = bundles(key)
    for order in ORDERS:
        assert B.handles[("tri", order)].edges == B.k["M"]   # loops gone, a pair stored twice counted once
        got = B.tri(order)
        B.check("tri", got, f"order {order}")
        assert not (got["tri"] >> np.uint64(32)).any()


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_core_numbers_with_and_without_chasing(bundles, key):
    B = bundles(key)
    assert B.handles["core"].edges == B.k["M"]
    for chase in CHASES:
        B.check("core", B.core(chase), f"chase {chase}")


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_truss_numbers(bundles, key):
    B = bundles(key)
    assert B.handles["truss"].edges == B.k["M"]
    B.check("truss", B.truss(), "")


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_greedy_colours_under_every_order(bundles, key):
    B = bundles(key)
    assert B.handles["color"].edges == B.k["M"]   # loops gone, a pair stored twice counted once
    for setting in R.COLOR_SETTINGS:
        ref = B.ref("color", setting)
        got, records = B.color(setting)
        print(f"{key_id(key)} (order, seed, prio) {setting}: colours {got['colors']} rounds {records[0]} sizes {records[1]}")
        B.check("color", got, f"(order, seed, prio) {setting}", ref)
        assert records == ref[1], (setting, records, ref[1])


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_spanning_forest_under_every_storing(bundles, key):
    B = bundles(key)
    for storing in B.weighted:
        ref = B.ref("msf", None, storing)
        assert B.handles[("msf", storing)].edges == ref[2]["M"]   # a stored +0.0 is no entry:
        if storing == "both ways":   # ... its pair is an edge through the opposite entry, or, where that is not stored, none
            assert ref[2]["M"] == B.k["M"]
        else:
            assert ref[2]["M"] < B.k["M"] == B.handles["color"].edges
        got, records = B.msf(storing)
        print(f"{key_id(key)} {storing}: edges {ref[2]['M']} tree edges {got['tree_edges']} rounds {records[0]} walked {records[1]}")
        B.check("msf", got, storing, ref)
        assert records == ref[1], (storing, records, ref[1])
        without, records = B.msf(storing, optional=False)
        B.check("msf", without, f"{storing}, every optional output None", ref)
        assert records == ref[1] and set(without) == {"in_msf", "tree_edges", "components", "complete"}


@pytest.mark.parametrize("key", KEYS, ids=key_id)
def test_greedy_matching_under_every_order(bundles, key):
    B = bundles(key)
    for storing in B.weighted:
        for setting in R.MATCH_SETTINGS:
            ref = B.ref("match", setting, storing)
            assert B.handles[("match", storing)].edges == ref[2]["M"]
            got, records = B.match(setting, storing)
            print(f"{key_id(key)} {storing} (heavy, seed) {setting}: pairs {got['pairs']} rounds {records[0]} walked {records[1]}")
            B.check("match", got, f"{storing} (heavy, seed) {setting}", ref)
            assert records == ref[1], (storing, setting, records, ref[1])
        without, records = B.match(R.MATCH_SETTINGS[-1], storing, optional=False)
        B.check("match", without, f"{storing}, in_match None", ref)
        assert records == ref[1] and "in_match" not in without


@pytest.mark.parametrize("key", RCM_KEYS, ids=key_id)
def test_rcm_orders_component_by_component(bundles, key):
    B = bundles(key)
    assert B.handles["rcm"].edges == B.k["M"]
    for setting in R.RCM_SETTINGS:
        ref = B.ref("rcm", setting)
        want = ref[0]
        assert want["steps"] <= MAX_RCM_STEPS, (key, setting, want["steps"])
        got, extra = B.rcm(setting)
        print(f"{key_id(key)} (sweeps, reverse) {setting}: components {got['components']} searches {got['sweeps_run']} steps {got['steps']}")
        B.check("rcm", got, f"(sweeps, reverse) {setting}", ref)
        same_as_rcm_gpu(dict(got, **extra), dict(want, M=ref[2]["M"], max_degree=ref[2]["max_degree"]), B.N)
        assert got["complete"] is True and np.array_equal(got["perm"][got["pos"]], np.arange(B.N))


# ------------------------------------------------------------------ 2. handles interleaved
@pytest.mark.parametrize("key,other", [(("digraphs", 4, "blocks"), ("undirected", 5, "strided")),
                                       (("undirected", 6, "strided"), ("digraphs", 3, "blocks")),
                                       (("undirected", 5, "blocks"), ("digraphs", 3, "strided"))],   # (both have all eleven)
                         ids=lambda k: key_id(k))
def test_a_handle_carries_nothing_over(bundles, key, other):
    """The eleven handles of one union round-robin, twice, the second round in reverse order, with the handles of another
    union used on the same engine between any two calls: every output equals that of the first call, and the reference.
    (rcm only where the union has its handle, see the module docstring; every other entry point is always compared.)"""
    B, O = bundles(key), bundles(other)
    first, others_first = {}, {}
    for turn, order in enumerate((ENTRY_POINTS, ENTRY_POINTS[::-1])):
        for i, what in enumerate(order):
            if what != "rcm" or B.has_rcm:   # (the only call passed over: rcm on a union that has no rcm handle)
                got = B.default_call(what)
                B.check(what, got, f"round {turn}")
                assert same(first.setdefault(what, got), got), (what, turn)
            between = ENTRY_POINTS[(i + 3) % len(ENTRY_POINTS)]   # (another entry point than the one just called)
            if between != "rcm" or O.has_rcm:
                got = O.default_call(between)
                O.check(between, got, f"between the calls of round {turn}")
                assert same(others_first.setdefault(between, got), got), (between, turn)

