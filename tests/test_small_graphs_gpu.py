"""The seven graph entry points on every small graph at once: the disjoint union of all digraphs with loops on 3 and
on 4 vertices and of all simple graphs on 4, 5 and 6 vertices, each union one matrix, one handle and one call per entry
point, under the two numberings of tests/small_graphs_ref.py (the vertices of a graph in neighbouring lanes / in
different workgroups), against the references written there from the definitions (tests/test_small_graphs_ref.py pins
them on the CPU).  Every union goes through all seven: the undirected ones, stored both ways, through bfs, sssp, scc and
wcc, where scc == wcc must hold as well; the digraph ones through tri, core and truss, whose graph is the symmetrised,
loop-free pattern -- almost every edge stored twice, and the loops must vanish.  For tri, core, truss and wcc the
undirected unions are stored ONE way (even graphs the upper triangle, odd graphs the lower): direction must not matter.

Every comparison is == on integer arrays or on uint32 views; there is no tolerance anywhere.  A mismatch is reported as
the smallest failing graph: its bit pattern, n, local adjacency and the local expected and actual rows.
"""
import numpy as np
import pytest

import small_graphs_ref as R
from sparseharness_amd.engine import Engine
from test_scc_gpu import SETTINGS as SCC_SETTINGS   # the four (trim, pivot) settings

pytestmark = pytest.mark.gpu

UNIONS = (("digraphs", 3), ("digraphs", 4), ("undirected", 4), ("undirected", 5), ("undirected", 6))
KEYS = tuple(u + (numbering,) for u in UNIONS for numbering in R.NUMBERINGS)
ENTRY_POINTS = ("bfs", "sssp", "scc", "wcc", "tri", "core", "truss")
TOP_DOWN, BOTTOM_UP, DEFAULT = (1.0, 0.0), (0.0, 0.0), (-1.0, -1.0)
# bucket widths: below the smallest non-zero weight (every distinct distance a bucket of its own), the default, one bucket
DELTAS = (float(R.SMALLEST_WEIGHT) / 2, -1.0, float("inf"))
SAMPLES = (0, 1, 2, 4)
ORDERS = (0, 1)
CHASES = (0, 4)
# caps no run here comes near (a BFS has at most 6 levels; the rounds are counted in the prints): they only keep the
# per-round arrays of the binding small
MAX_LEVELS, MAX_ROUNDS = 64, 1 << 14


def key_id(key):
    return f"{key[0]}{key[1]}-{key[2]}"


class Bundle:
    """One union under one numbering: its CSR arrays, the references, and the handles of all seven entry points (tri
    has one per order), alive together until the module is done."""

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

    def default_call(self, what):
        """-> the outputs of one call of an entry point at its default setting (what the interleaving test compares)."""
        got = getattr(self, what)()
        return got[0] if isinstance(got, tuple) else got

    # ---- comparing
    def check(self, what, got, setting):
        """Every output of `got` equals the reference's; a vector that differs is told as the smallest failing graph."""
        want = self.want[what]
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
            else:
                inputs = {}
                if what == "bfs":
                    inputs = {"source": self.sources}
                if what == "sssp":   # (an entry at (r, c) weighs small_graphs_ref.TABLE[r, c] in every graph)
                    inputs = {"x0": self.x0}
                show = (lambda v: v.view(np.float32)) if name == "dist" else None   # compared as bits, shown as floats
                text = R.explain_vertices(self.A, self.numbering, expected, value, name in ("parent", "pred", "comp"), inputs, show)
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


# ------------------------------------------------------------------ 2. handles interleaved
@pytest.mark.parametrize("key,other", [(("digraphs", 4, "blocks"), ("undirected", 5, "strided")),
                                       (("undirected", 6, "strided"), ("digraphs", 3, "blocks"))],
                         ids=lambda k: key_id(k))
def test_a_handle_carries_nothing_over(bundles, key, other):
    """The seven handles of one union round-robin, twice, the second round in reverse order, with the handles of another
    union used on the same engine between any two calls: every output equals that of the first call, and the reference."""
    B, O = bundles(key), bundles(other)
    first, others_first = {}, {}
    for turn, order in enumerate((ENTRY_POINTS, ENTRY_POINTS[::-1])):
        for i, what in enumerate(order):
            got = B.default_call(what)
            B.check(what, got, f"round {turn}")
            assert same(first.setdefault(what, got), got), (what, turn)
            between = ENTRY_POINTS[(i + 3) % len(ENTRY_POINTS)]   # (another entry point than the one just called)
            got = O.default_call(between)
            O.check(between, got, f"between the calls of round {turn}")
            assert same(others_first.setdefault(between, got), got), (between, turn)

