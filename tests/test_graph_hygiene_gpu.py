"""What a graph or worklist call may read and write: its operands -- `rows` elements of each (`edges` for sh_truss), no
more -- and its handle.  GPU AddressSanitizer's class of error, caught by construction: every comparison is == on 32-bit
words against the references of tests/graph_hygiene_shapes.py (tests/test_graph_hygiene_cpu.py proves that the shapes
make a word written too far, left unwritten or read from a guard visible).

Tier 1, the production library.  Every vector operand of sh_bfs_levels, sh_sssp, sh_scc, sh_wcc, sh_tri, sh_core,
sh_truss, sh_color, sh_msf, sh_match, sh_rcm and sh_iterate_frontier is a view (sh_vec_wrap) between 256 guard words on
either side, read back whole after the call.  A call with operands o_0 .. o_j runs four times on one handle; in run k
operand o_i starts (i + k) % 4 words behind a 256-byte boundary.  Each run is made with views of exactly the required
length and again with 3 elements more, which must still hold what they held.  Outputs are prefilled with 0xDEADBEEF
between guards of it; the guards of an input mean something if they are read (a source for the searches, the semiring's
poison for the iteration, a priority above every vertex's around prio of sh_color).  Asserted per
call: every output vector and every scalar or record that does not depend on the setting equals the reference, no guard
word changed, every input is bit for bit what was uploaded.  A run cut short (max_levels / max_rounds / max_steps /
max_iters = 1, on the wheel) leaves guards and tail alone as well, and sh_sssp leaves `pred` untouched; sh_color, sh_msf,
sh_match and sh_rcm then leave what the header says (-1 for a vertex without a colour, a component, a mate or a position,
the tree edges and pairs of the first round), compared with the max_rounds / max_steps forms of their references.  The
header states no alignment rule for the operands of these four: the rotation through all four word offsets pins that.
The small operations -- sh_vec_fill, sh_vec_copy, sh_bits_from_column, sh_bits_to_column -- on views of odd lengths at
every word offset: neither has an alignment rule, and the test pins that.

Tier 2, the tools library: the same guarded calls of all twelve with every per-call array of the handle poisoned before
each call (sh_debug_poison_graph, csrc/debug_graph_tools.h)."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import bfs_ref
import graph_hygiene_shapes as S
import hygiene_shapes as HS
import small_graphs_ref as R
from guarded import DEAD, Dev, _not_halted, call, same_bits   # noqa: F401 (the fixture is used by being here)
from sparseharness_amd import abi
from sparseharness_amd.engine import Engine, EngineError
from test_plan_limits_gpu import Tools

pytestmark = pytest.mark.gpu

TOP_DOWN, BOTTOM_UP, DEFAULT = (1.0, 0.0), (0.0, 0.0), (-1.0, -1.0)   # the shares of tests/test_small_graphs_gpu.py
SCC_SETTINGS = ((1, 1), (0, 0))
SAMPLES, ORDERS, CHASES = (0, 2), (0, 1), (0, 4)
MAX_LEVELS, MAX_ROUNDS = 64, 1 << 14   # caps no complete run here comes near
EXTRAS = (0, S.EXTRA)
_t0 = time.time()


@contextlib.contextmanager
def using(lib):
    """sparseharness_amd.engine calls whatever abi.load() returns: inside, that is `lib`."""
    abi.load()
    old, abi._lib = abi._lib, lib
    try:
        yield
    finally:
        abi._lib = old


class Ctx:
    """One library, one engine on it, and the handles of every shape, made at first use and kept until the module is done."""

    def __init__(self, lib):
        self.lib = lib
        with using(lib):
            self.eng = Engine(0)
        self.dev = Dev(lib, self.eng.h)
        self.made, self.mats = {}, {}

    def handles(self, name):
        if name not in self.made:
            s, eng = S.shape(name), self.eng
            ones, ones1 = np.ones(len(s.ci), np.float32), np.ones(len(s.ci1), np.float32)
            with using(self.lib):
                h = dict(bfs=eng.bfs_graph(s.rp, s.ci, ones), sssp=eng.sssp_graph(s.rp, s.ci, s.val), scc=eng.scc_graph(s.rp, s.ci, ones),
                         wcc=eng.wcc_graph(s.rp1, s.ci1, ones1), core=eng.core_graph(s.rp1, s.ci1, ones1),
                         truss=eng.truss_graph(s.rp1, s.ci1, ones1), color=call(eng.color_graph, s.rp1, s.ci1, ones1),
                         rcm=call(eng.rcm_graph, s.rp1, s.ci1, ones1), msf=call(eng.msf_graph, s.rp, s.ci, s.wval),
                         match=call(eng.match_graph, s.rp, s.ci, s.wval))
                for order in ORDERS:
                    h[("tri", order)] = eng.tri_graph(s.rp1, s.ci1, ones1, order=order)
                assert h["truss"].edges == h["core"].edges == h[("tri", 0)].edges == h["color"].edges == h["rcm"].edges == s.M
                assert h["msf"].edges == h["match"].edges == s.Mw
            self.made[name] = h
        return self.made[name]

    def frontier(self, name, sr, plan):
        key = (name, sr, plan)
        if key not in self.mats:
            s = S.shape(name)
            va = S.frontier_case(name, sr)[0]
            with using(self.lib):
                A = self.eng.upload_csr(s.rows, s.rows, s.rp, s.ci, va, plan=plan)
                assert A.describe().startswith("stream" if plan == 1 else "tiled"), A.describe()
                self.mats[key] = (A, self.eng.frontier(A, s.rp, s.ci, va))
        return self.mats[key]

    def close(self):
        with using(self.lib):
            for A, F in self.mats.values():
                F.free()
                A.free()
            for h in self.made.values():
                for g in h.values():
                    g.free()
            self.eng.close()

    # ---- operands
    def inp(self, data, k, guard, extra=0):
        """An input of len(data) + extra elements at word offset k, the extra elements and the guards holding `guard`."""
        words = np.concatenate([HS.bits(data).ravel(), np.full(extra, guard, np.uint32)])
        g = self.dev.guarded(words, k % 4, guard)
        g.uploaded = words
        return g

    def out(self, n, k, extra=0):
        """An output of n + extra elements at word offset k, prefilled with 0xDEADBEEF between guards of it."""
        g = self.dev.guarded(np.full(n + extra, DEAD, np.uint32), k % 4, DEAD)
        g.n_out = n
        return g


def unchanged(view, what):
    same_bits(view.read(what), view.uploaded, what + " was written")


def written(view, want, what):
    """The view's first n_out elements are `want`, bit for bit, the guards intact and the tail still 0xDEADBEEF."""
    got = view.read(what)
    tail = got[view.n_out:]
    assert (tail == DEAD).all(), f"{what}: {int((tail != DEAD).sum())} of the {len(tail)} elements behind the vector were written: {[hex(v) for v in tail]}"
    same_bits(got[:view.n_out], want, what)


def untouched(view, what):
    got = view.read(what)
    assert (got == DEAD).all(), f"{what}: {int((got != DEAD).sum())} words were written, first at {np.flatnonzero(got != DEAD)[:6].tolist()}"


def only_head_written(view, what):
    """A run that was cut short: the guards and the tail are intact (the head holds what the run got to)."""
    got = view.read(what)
    assert (got[view.n_out:] == DEAD).all(), f"{what}: the elements behind the vector were written: {[hex(v) for v in got[view.n_out:]]}"
    return got[:view.n_out]


def free(*views):
    for v in views:
        if v is not None:
            v.free()


@pytest.fixture(scope="module")
def prod():
    c = Ctx(abi.load())
    yield c
    c.close()
    print(f"tests/test_graph_hygiene_gpu.py: {time.time() - _t0:.1f} s since import")


def runs():
    """(k, extra) of the eight runs of a call: four rotations of the offsets, exact views and views of 3 elements more."""
    return [(k, extra) for extra in EXTRAS for k in range(4)]


# ------------------------------------------------------------------ one guarded call of each entry point
def bfs_bookkeeping(s, want):
    """What bfs_ref.predict_modes and the per-step edge counts need, from the reference's levels: m_L = the out-list lengths
    of level L, and the entries of the rows still unvisited before step L (every stored entry of these shapes is an edge)."""
    level, c, r = want["level"], s.ci, bfs_ref.rows_of_entries(s.rp)
    outdeg, indeg = np.bincount(c, minlength=s.rows), np.bincount(r, minlength=s.rows)
    b = bfs_ref.Bfs()
    b.n, b.E, b.sizes, b.steps = s.rows, len(c), want["sizes"], len(want["sizes"]) - 1
    b.m = [int(outdeg[level == L].sum()) for L in range(b.steps + 1)]
    b.open_entries = [int(indeg[(level == -1) | (level > L)].sum()) for L in range(b.steps)]
    return b


def bfs(c, name, st, shares, with_parent, k, extra, before=None, max_levels=MAX_LEVELS, want=None):
    s, want = S.shape(name), want or st.bfs
    what = f"sh_bfs_levels {name} {st.label} shares {shares} parent {with_parent} run {k} extra {extra} max_levels {max_levels}"
    x, lv = c.inp(st.sources, k, S.BFS_X0_GUARD, extra), c.out(s.rows, k + 1, extra)
    pv = c.out(s.rows, k + 2, extra) if with_parent else None
    try:
        if before:
            before("bfs", c.handles(name)["bfs"], what)
        with using(c.lib):
            depth, reached, complete, modes, sizes, edges, _, _ = call(c.eng.bfs_levels, c.handles(name)["bfs"], x, lv, pv, max_levels=max_levels,
                                                                       up_share=shares[0], down_share=shares[1])
        written(lv, want["level"], what + ": level")
        if with_parent:
            written(pv, want["parent"], what + ": parent")
        assert (depth, reached, complete, sizes.tolist()) == (want["depth"], want["reached"], want["complete"], want["sizes"]), \
            (what, depth, reached, complete, sizes.tolist())
        # the direction of every step is the header's rule on the reference; a top-down step looks at the out-lists of its
        # frontier, no entry more (a stale queue entry or bitmap word would add some), a bottom-up step at no more than
        # the entries of the unvisited rows
        b = bfs_bookkeeping(s, want)
        assert list(modes) == bfs_ref.predict_modes(b, *shares) and len(edges) == b.steps, (what, list(modes))
        for L in range(b.steps):
            if modes[L] == 0:
                assert edges[L] == b.m[L], (what, L, list(edges), b.m)
            else:
                assert b.sizes[L + 1] <= edges[L] <= b.open_entries[L], (what, L, list(edges), b.sizes, b.open_entries)
        unchanged(x, what + ": x0")
    finally:
        free(x, lv, pv)


def sssp(c, name, st, delta, with_pred, k, extra, before=None, max_rounds=MAX_ROUNDS):
    s, want = S.shape(name), st.sssp
    what = f"sh_sssp {name} {st.label} delta {delta} pred {with_pred} run {k} extra {extra} max_rounds {max_rounds}"
    x, dv = c.inp(st.x0, k, S.SSSP_X0_GUARD, extra), c.out(s.rows, k + 1, extra)
    pv = c.out(s.rows, k + 2, extra) if with_pred else None
    try:
        if before:
            before("sssp", c.handles(name)["sssp"], what)
        with using(c.lib):
            res = call(c.eng.sssp, c.handles(name)["sssp"], x, dv, pv, delta=delta, max_rounds=max_rounds)
        reached, complete = res[2], res[3]
        if max_rounds == MAX_ROUNDS:
            written(dv, want["dist"], what + ": dist")
            if with_pred:
                written(pv, want["pred"], what + ": pred")
            assert (reached, complete) == (want["reached"], True), (what, reached, complete)
        else:   # cut short: pred is written by a complete run only
            assert not complete, what
            only_head_written(dv, what + ": dist")
            untouched(pv, what + ": pred of a run that was cut short")
        unchanged(x, what + ": x0")
    finally:
        free(x, dv, pv)


def components(c, name, which, setting, k, extra, before=None, cap=MAX_ROUNDS):
    """sh_scc (setting = (trim, pivot)) or sh_wcc (setting = sample)."""
    s, want = S.shape(name), S.shape(name).want[which]
    what = f"sh_{which} {name} setting {setting} run {k} extra {extra} cap {cap}"
    cv = c.out(s.rows, k, extra)
    try:
        if before:
            before(which, c.handles(name)[which], what)
        with using(c.lib):
            if which == "scc":
                res = call(c.eng.scc, c.handles(name)["scc"], cv, trim=setting[0], pivot=setting[1], max_steps=cap)
                count, complete = res[0], res[5]
            else:
                res = call(c.eng.wcc, c.handles(name)["wcc"], cv, sample=setting, max_rounds=cap)
                count, complete = res[0], res[3]
        if cap == MAX_ROUNDS:
            assert complete, what
        if complete:
            written(cv, want["comp"], what + ": comp")
            assert count == want["components"], (what, count)
        else:
            only_head_written(cv, what + ": comp")
    finally:
        free(cv)


def tri(c, name, order, with_tri, with_deg, k, extra, before=None):
    """tri needs 8-byte alignment: it sits at word 0 and 2 in turn while deg rotates through all four offsets."""
    s, want = S.shape(name), S.shape(name).want["tri"]
    what = f"sh_tri {name} order {order} tri {with_tri} deg {with_deg} run {k} extra {extra}"
    tv = c.out(2 * s.rows, 2 * (k % 2), 2 * extra) if with_tri else None
    dv = c.out(s.rows, k + 1, extra) if with_deg else None
    try:
        if before:
            before("tri", c.handles(name)[("tri", order)], what)
        with using(c.lib):
            total, _, _ = call(c.eng.triangles, c.handles(name)[("tri", order)], tv, dv)
        assert total == want["triangles"], (what, total)
        if with_tri:
            written(tv, want["tri"], what + ": tri")
        if with_deg:
            written(dv, want["deg"], what + ": deg")
    finally:
        free(tv, dv)


def core(c, name, chase, with_deg, k, extra, before=None, max_rounds=None):
    s, want = S.shape(name), S.shape(name).want["core"]
    what = f"sh_core {name} chase {chase} deg {with_deg} run {k} extra {extra} max_rounds {max_rounds}"
    cv = c.out(s.rows, k, extra)
    dv = c.out(s.rows, k + 1, extra) if with_deg else None
    try:
        if before:
            before("core", c.handles(name)["core"], what)
        with using(c.lib):
            res = call(c.eng.core_numbers, c.handles(name)["core"], cv, dv, chase=chase, max_rounds=max_rounds)
        degeneracy, complete = res[0], res[3]
        if max_rounds is None:
            assert complete and degeneracy == want["degeneracy"], (what, complete, degeneracy)
            written(cv, want["core"], what + ": core")
        else:
            assert not complete, what
            only_head_written(cv, what + ": core")
        if with_deg:
            written(dv, want["deg"], what + ": deg")
    finally:
        free(cv, dv)


TRUSS_VECTORS = ("truss", "support", "edge_u", "edge_v")


def truss(c, name, with_optional, k, extra, before=None, max_rounds=None):
    s, want = S.shape(name), S.shape(name).want["truss"]
    what = f"sh_truss {name} optional vectors {with_optional} run {k} extra {extra} max_rounds {max_rounds}"
    G = c.handles(name)["truss"]
    vecs = [c.out(s.M, k + i, extra) if (i == 0 or with_optional) else None for i in range(4)]
    try:
        if before:
            before("truss", G, what)
        with using(c.lib):
            res = call(c.eng.truss_numbers, G, *vecs, max_rounds=max_rounds)
            assert G.edges == want["edges"]
        max_truss, complete, triangles = res[0], res[3], res[4]
        assert triangles == want["triangles"], (what, triangles)
        for vec_name, v in zip(TRUSS_VECTORS, vecs):
            if v is None:
                continue
            if vec_name == "truss" and max_rounds is not None:
                assert not complete, what
                only_head_written(v, what + ": truss")
            else:   # support and the ends are valid after the support pass, however short the run was cut
                written(v, want[vec_name], f"{what}: {vec_name}")
        if max_rounds is None:
            assert complete and max_truss == want["max_truss"], (what, complete, max_truss)
    finally:
        free(*vecs)


def color(c, name, setting, k, extra, before=None, max_rounds=None):
    """prio, where the setting has one, is a guarded input: its guards and tail hold a priority above every vertex's."""
    s, (order, seed, with_prio) = S.shape(name), setting
    want = (s.want if max_rounds is None else s.cut)["color"][setting]
    what = f"sh_color {name} (order, seed, prio) {setting} run {k} extra {extra} max_rounds {max_rounds}"
    cv = c.out(s.rows, k, extra)
    pv = c.inp(s.prio, k + 1, S.PRIO_GUARD, extra) if with_prio else None
    try:
        if before:
            before("color", c.handles(name)["color"], what)
        with using(c.lib):
            res = call(c.eng.greedy_colors, c.handles(name)["color"], cv, pv, order=order, seed=seed, max_rounds=max_rounds)
        colors, rounds, complete, coloured = res[:4]
        written(cv, want["color"], what + ": color")   # (a run cut short leaves -1 for every vertex without a colour)
        assert (colors, rounds, complete) == (want["colors"], want["rounds"], max_rounds is None), (what, colors, rounds, complete)
        assert coloured == int((want["color"] >= 0).sum()), (what, coloured)
        if with_prio:
            unchanged(pv, what + ": prio")
    finally:
        free(cv, pv)


MSF_VECTORS = ("in_msf", "comp", "edge_u", "edge_v", "weight")
MATCH_VECTORS = ("mate", "in_match", "edge_u", "edge_v", "weight")
RCM_VECTORS = ("perm", "pos", "level")


def msf(c, name, with_optional, k, extra, before=None, max_rounds=33):
    s = S.shape(name)
    want = (s.want if max_rounds == 33 else s.cut)["msf"]
    what = f"sh_msf {name} optional vectors {with_optional} run {k} extra {extra} max_rounds {max_rounds}"
    G = c.handles(name)["msf"]
    vecs = [c.out(s.rows if nm == "comp" else s.Mw, k + i, extra) if (i == 0 or with_optional) else None for i, nm in enumerate(MSF_VECTORS)]
    try:
        if before:
            before("msf", G, what)
        with using(c.lib):
            res = call(c.eng.spanning_forest, G, *vecs, max_rounds=max_rounds)
        for nm, v in zip(MSF_VECTORS, vecs):   # (cut short: the tree edges of the rounds run, comp -1 everywhere)
            if v is not None:
                written(v, want[nm], f"{what}: {nm}")
        assert res[:2] == (want["tree_edges"], want["components"]) and res[3] == (max_rounds == 33), (what, res[:4])
    finally:
        free(*vecs)


def match(c, name, setting, with_optional, k, extra, before=None, max_rounds=MAX_ROUNDS):
    s = S.shape(name)
    want = (s.want if max_rounds == MAX_ROUNDS else s.cut)["match"][setting]
    what = f"sh_match {name} (heavy, seed) {setting} optional vectors {with_optional} run {k} extra {extra} max_rounds {max_rounds}"
    G = c.handles(name)["match"]
    vecs = [c.out(s.rows if nm == "mate" else s.Mw, k + i, extra) if (i == 0 or with_optional) else None for i, nm in enumerate(MATCH_VECTORS)]
    try:
        if before:
            before("match", G, what)
        with using(c.lib):
            res = call(c.eng.matching, G, vecs[0], setting[0], setting[1], *vecs[1:], max_rounds=max_rounds)
        for nm, v in zip(MATCH_VECTORS, vecs):   # (cut short: the pairs of the rounds run, -1 for everybody else)
            if v is not None:
                written(v, want[nm], f"{what}: {nm}")
        assert (res[0], res[2]) == (want["pairs"], max_rounds == MAX_ROUNDS), (what, res[:3])
    finally:
        free(*vecs)


def rcm(c, name, setting, with_optional, k, extra, before=None, max_steps=None):
    s = S.shape(name)
    want = (s.want if max_steps is None else s.cut)["rcm"][setting]
    what = f"sh_rcm {name} (sweeps, reverse) {setting} optional vectors {with_optional} run {k} extra {extra} max_steps {max_steps}"
    G = c.handles(name)["rcm"]
    vecs = [c.out(s.rows, k + i, extra) if (i == 0 or with_optional) else None for i in range(3)]
    try:
        if before:
            before("rcm", G, what)
        with using(c.lib):
            res = call(c.eng.rcm_order, G, *vecs, sweeps=setting[0], reverse=setting[1], max_steps=max_steps)
        for nm, v in zip(RCM_VECTORS, vecs):   # (cut short: -1 in the rest of perm, and for a vertex without a position)
            if v is not None:
                written(v, want[nm], f"{what}: {nm}")
        assert res[:8] == tuple(want[f] for f in S.RCM_SCALARS), (what, res[:8])
        for f, got in zip(("kind", "size", "edges"), res[8:11]):
            assert np.array_equal(got, want[f]), (what, f)
    finally:
        free(*vecs)


def frontier(c, name, sr, plan, share, k, extra, before=None, max_iters=S.FRONTIER_CAP):
    s = S.shape(name)
    va, x0, want, launches, converged = S.frontier_case(name, sr)
    what = f"sh_iterate_frontier {name} {HS.SR_NAME[sr]} plan {plan} dense_share {share} run {k} extra {extra} max_iters {max_iters}"
    A, F = c.frontier(name, sr, plan)
    poison = HS.POISON[sr]
    x, y0 = c.inp(x0, k, poison, extra), c.inp(x0, k + 1, poison, extra)
    sc = c.inp(np.full(s.rows, poison, np.uint32), k + 2, poison, extra)
    try:
        if before:
            before("frontier", F, what)
        with using(c.lib):
            it, conv, modes, _, _, _, _ = call(c.eng.iterate_frontier, sr, A, F, x, y0, sc, *S.FRONTIER_SCALARS[sr], delta=S.DELTA,
                                               max_iters=max_iters, dense_share=share)
        got = x.read(what + ": x")
        tail = sc.read(what + ": scratch")[s.rows:]
        assert (got[s.rows:] == poison).all() and (tail == poison).all(), f"{what}: the elements behind x or scratch were written"
        unchanged(y0, what + ": y0")
        if max_iters == S.FRONTIER_CAP:
            assert (it, conv) == (launches, converged), (what, it, conv)
            same_bits(got[:s.rows], want, what + ": x")
            assert modes == ([0] * it if share == 0.0 else [0, 0] + [1] * (it - 2)), (what, modes)
        else:
            assert (it, conv) == (max_iters, False), (what, it, conv)
    finally:
        free(x, y0, sc)


# ------------------------------------------------------------------ Tier 1: guards, offsets, lengths
def sssp_deltas(name):
    """A bucket width below the smallest weight (every distinct distance a bucket of its own), and one bucket."""
    return (0.25 if name == "wheel" else float(R.SMALLEST_WEIGHT) / 2, float("inf"))


@pytest.mark.parametrize("name", S.NAMES)
def test_bfs_levels_between_guards(prod, name):
    for st in S.shape(name).starts:
        for shares in (TOP_DOWN, BOTTOM_UP, DEFAULT):
            for with_parent in (True, False):
                for k, extra in runs():
                    bfs(prod, name, st, shares, with_parent, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_sssp_between_guards(prod, name):
    for st in S.shape(name).starts:
        for delta in sssp_deltas(name):
            for with_pred in (True, False):
                for k, extra in runs():
                    sssp(prod, name, st, delta, with_pred, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_scc_between_guards(prod, name):
    for setting in SCC_SETTINGS:
        for k, extra in runs():
            components(prod, name, "scc", setting, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_wcc_between_guards(prod, name):
    for sample in SAMPLES:
        for k, extra in runs():
            components(prod, name, "wcc", sample, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_tri_between_guards(prod, name):
    for order in ORDERS:
        for with_tri, with_deg in ((True, True), (True, False), (False, True)):
            for k, extra in runs():
                tri(prod, name, order, with_tri, with_deg, k, extra)


@pytest.mark.parametrize("name", ("u5x13-blocks", "wheel"))
def test_tri_refuses_a_count_vector_off_its_8_byte_boundary(prod, name):
    s = S.shape(name)
    for offset in (1, 3):
        for k in range(4):
            tv, dv = prod.out(2 * s.rows, offset), prod.out(s.rows, k)
            try:
                with using(prod.lib), pytest.raises(EngineError) as err:
                    call(prod.eng.triangles, prod.handles(name)[("tri", 1)], tv, dv)
                assert err.value.code == abi.SH_EINVAL, err.value
                untouched(tv, f"sh_tri {name}: tri at word {offset}, refused")
                untouched(dv, f"sh_tri {name}: deg at word {k} beside a refused tri")
            finally:
                free(tv, dv)


@pytest.mark.parametrize("name", S.NAMES)
def test_core_between_guards(prod, name):
    for chase in CHASES:
        for with_deg in (True, False):
            for k, extra in runs():
                core(prod, name, chase, with_deg, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_truss_between_guards(prod, name):
    for with_optional in (True, False):
        for k, extra in runs():
            truss(prod, name, with_optional, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_color_between_guards(prod, name):
    for setting in S.COLOR_SETTINGS:   # (with and without prio, the optional operand)
        for k, extra in runs():
            color(prod, name, setting, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_msf_between_guards(prod, name):
    for with_optional in (True, False):
        for k, extra in runs():
            msf(prod, name, with_optional, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_match_between_guards(prod, name):
    for setting in S.MATCH_SETTINGS:
        for with_optional in (True, False):
            for k, extra in runs():
                match(prod, name, setting, with_optional, k, extra)


@pytest.mark.parametrize("name", S.NAMES)
def test_rcm_between_guards(prod, name):
    """u5x1023 has 1398 components with edges, and sh_rcm pays per step: 10 824 steps a call at sweeps = 8, 3608 at 0.
    Its eight runs of four calls took 4.5 s on an MI355X, so there two runs stand for the eight: offset 1 at the exact
    length and offset 3 with 3 elements more.  Every other shape keeps all eight."""
    some = [(1, 0), (3, S.EXTRA)] if name.startswith("u5x1023") else runs()
    for setting in S.RCM_SETTINGS:
        for with_optional in (True, False):
            for k, extra in some:
                rcm(prod, name, setting, with_optional, k, extra)


@pytest.mark.parametrize("sr", S.FRONTIER_SEMIRINGS, ids=HS.SR_NAME.get)
@pytest.mark.parametrize("name", S.FRONTIER_NAMES)
def test_iterate_frontier_between_guards(prod, name, sr):
    for plan in (1, 2):
        for share in (0.0, 1.0):
            for k, extra in runs():
                frontier(prod, name, sr, plan, share, k, extra)


def test_a_run_cut_short_stays_inside_its_vectors(prod):
    """One level, round, step or launch on the wheel, views of rows + 3 elements, at every rotation of the offsets."""
    s = S.shape("wheel")
    for k in range(4):
        for st in s.starts:
            for shares in (TOP_DOWN, BOTTOM_UP):
                bfs(prod, "wheel", st, shares, True, k, S.EXTRA, max_levels=1, want=st.bfs_cut)
        sssp(prod, "wheel", s.starts[0], sssp_deltas("wheel")[0], True, k, S.EXTRA, max_rounds=1)
        components(prod, "wheel", "scc", (1, 1), k, S.EXTRA, cap=1)
        components(prod, "wheel", "wcc", 0, k, S.EXTRA, cap=1)
        core(prod, "wheel", 0, True, k, S.EXTRA, max_rounds=1)
        truss(prod, "wheel", True, k, S.EXTRA, max_rounds=1)
        for setting in S.COLOR_SETTINGS:
            color(prod, "wheel", setting, k, S.EXTRA, max_rounds=1)
        msf(prod, "wheel", True, k, S.EXTRA, max_rounds=1)
        for setting in S.MATCH_SETTINGS:
            match(prod, "wheel", setting, True, k, S.EXTRA, max_rounds=1)
        for setting in S.RCM_SETTINGS:
            rcm(prod, "wheel", setting, True, k, S.EXTRA, max_steps=1)
        for sr in S.FRONTIER_SEMIRINGS:
            frontier(prod, "wheel", sr, 1, 1.0, k, S.EXTRA, max_iters=1)


# ------------------------------------------------------------------ the small operations
PATTERN = 0x5EED1E55


@pytest.mark.parametrize("n", (1, 255, 257))
def test_vec_fill_and_copy_on_views(prod, n):
    dev, rng = prod.dev, np.random.default_rng(n)
    for k in range(4):
        v = prod.out(n, k)
        src = prod.inp(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), k + 1, 0x0BADF00D)
        try:
            dev.ok(dev.lib.sh_vec_fill(dev.h, v.v, PATTERN))
            assert (v.read(f"sh_vec_fill of {n} elements at word {k}") == PATTERN).all()
            dev.ok(dev.lib.sh_vec_copy(dev.h, v.v, src.v))
            same_bits(v.read(f"sh_vec_copy of {n} elements to word {k}"), src.uploaded, f"sh_vec_copy of {n} elements from word {(k + 1) % 4} to word {k}")
            unchanged(src, f"sh_vec_copy of {n} elements: the source")
        finally:
            free(v, src)


@pytest.mark.parametrize("n", (1, 255, 257, 1023))
@pytest.mark.parametrize("words", (1, 2, 4, 8))
def test_bits_columns_on_views(prod, words, n):
    dev, rng = prod.dev, np.random.default_rng(1000 * words + n)
    for i, source in enumerate(sorted({0, 31, 32 * (words - 1), 32 * words - 1})):
        for k in range(4):
            extra = S.EXTRA * (k % 2)   # a B longer than n * words and a v longer than n in every other run
            b0 = rng.integers(0, 1 << 32, n * words + extra, dtype=np.uint64).astype(np.uint32)
            v0 = np.where(rng.random(n + extra) < 0.5, 0, rng.integers(1, 1 << 32, n + extra, dtype=np.uint64)).astype(np.uint32)
            what = f"words {words} n {n} source {source}, B at word {k}, v at word {(k + i + 1) % 4}"
            B, v, col = prod.inp(b0, k, 0x0BADF00D), prod.inp(v0, k + i + 1, 0x0BADF00D), prod.out(n, k + i + 2, extra)
            try:
                dev.ok(dev.lib.sh_bits_from_column(dev.h, v.v, n, words, source, B.v))
                want = b0.copy()
                at, bit = np.arange(n) * words + source // 32, np.uint32(1 << (source % 32))
                want[at] = np.where(v0[:n] != 0, want[at] | bit, want[at] & ~bit)
                same_bits(B.read("sh_bits_from_column " + what + ": B"), want, "sh_bits_from_column " + what)
                unchanged(v, "sh_bits_from_column " + what + ": v")
                dev.ok(dev.lib.sh_bits_to_column(dev.h, B.v, n, words, source, col.v))
                written(col, (v0[:n] != 0).astype(np.uint32), "sh_bits_to_column " + what)
                same_bits(B.read("sh_bits_to_column " + what + ": B"), want, "sh_bits_to_column " + what + ": B was written")
            finally:
                free(B, v, col)


# ------------------------------------------------------------------ Tier 2: what a call must initialise itself, poisoned
# sh_debug_poison_graph (csrc/debug_graph_tools.h) fills, before a call, every array of the handle that a call reads only
# after writing it: data words with 0xFFFFFFFF or 0, queues and work lists with a valid vertex or edge id whose
# consumption would change the answer, piece lists with the first piece of that vertex (DESIGN.md "Graph and worklist
# hygiene" lists the arrays and the ones left out).
KIND = {"frontier": 0, "bfs": 1, "sssp": 2, "scc": 3, "wcc": 4, "tri": 5, "core": 6, "truss": 7, "color": 8, "msf": 9, "match": 10, "rcm": 11}
N_SIZES = 12
TIER2_NAMES = ("u5x51-strided", "wheel")
ONES, ZERO = 0xFFFFFFFF, 0x00000000
_printed = set()


@pytest.fixture(scope="module")
def tools():
    t = Tools()
    t.lib.sh_debug_poison_graph.restype = C.c_int
    t.lib.sh_debug_poison_graph.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]
    c = Ctx(t.lib)
    yield c
    c.close()
    t.close()


def owned_bytes(kind, s, edges):
    """The bytes of every array sh_debug_poison_graph fills, whole, in its order (an array is 16 bytes at least)."""
    arr, r, m = (lambda b: max(b, 16)), 4 * s.rows, 4 * s.M
    words = 4 * ((s.rows + 31) // 32)
    pieces = arr(8 * (edges // 1024 + 1))
    return {"frontier": [512, arr(r), arr(r), arr(r), arr(8 * (edges // 1024 + 1)), arr(8 * (edges // 2048 + 1))],
            "scc": [2048 + 16384, 16384, arr(r), arr(r), arr(r), arr(r), arr(r), pieces, pieces, pieces, pieces],
            "wcc": [2048 + 2 * 16384, arr(r), arr(r), pieces, pieces],
            "bfs": [2048 + 16384, arr(words), arr(words), arr(r), arr(r), pieces, pieces],
            "sssp": [2048 + 16384 + 4096, arr(r), arr(r), arr(r), arr(r), arr(r), pieces, pieces],
            "tri": [2 * 16384],
            "core": [2048 + 2 * 16384, arr(r), arr(r), arr(r), arr(8 * (2 * s.M // 1024 + 1)), arr(8 * (2 * s.M // 1024 + 1))],
            "truss": [2048 + 3 * 16384, arr(m), arr(m), arr(m), arr(m)],
            "color": [1024 + 16384, arr(r), arr(r), arr(r)],
            "msf": [1024 + 2 * 16384, arr(2 * r), arr(r), arr(r), arr(4 * edges), arr(4 * edges)],
            "match": [1024 + 16384, arr(2 * r), arr(4 * edges), arr(4 * edges)],
            "rcm": [1024 + 16384 + 32768] + [arr(r)] * 6}[kind]


def index_word(kind, s):
    """A valid id whose consumption would change the answer: a vertex the searches leave unreached (on the wheel, which is
    connected, one two levels from the rim source; for sh_iterate_frontier it is the vertex whose word changes last or
    never), a vertex of the largest core number, an edge of the largest truss number.  sh_scc and sh_wcc: vertex 0.  Every
    reference label is the largest index of its component, so comp[v] >= v > 0 for every other vertex: a parent word or a
    list entry 0 that a call took for its own would hang a vertex under 0 or settle vertex 0 out of turn."""
    if kind in ("scc", "wcc"):
        return 0
    if kind in ("bfs", "sssp", "frontier"):
        level = s.starts[0].bfs["level"]
        return int(np.flatnonzero(level == -1)[-1]) if (level == -1).any() else int(np.flatnonzero(level == 2)[-1])
    if kind == "truss":
        return int(np.argmax(s.want["truss"]["truss"]))
    if kind in ("msf", "match"):
        # one word for two id spaces, so below min(rows, edges).  sh_msf: as a vertex one that is not the largest of its
        # component (a parent word taken for the call's own hangs a tree under it: comp differs), as an edge one outside
        # the forest (taken from a stale list and chosen, in_msf differs).  sh_match: an edge outside the matching under
        # every setting run here.
        lim = min(s.rows, s.Mw)
        if kind == "msf":
            ok = (s.want["msf"]["in_msf"][:lim] == 0) & (s.want["msf"]["comp"][:lim] != np.arange(lim))
        else:
            ok = np.all([w["in_match"][:lim] == 0 for w in s.want["match"].values()], axis=0)
        return int(np.flatnonzero(ok)[-1])
    return int(np.argmax(s.want["core"]["core"]))   # sh_core, and sh_color and sh_rcm: coloured or numbered twice, out of turn


def poisoner(c, name, data_word):
    def before(kind, G, what):
        s = S.shape(name)
        sizes = (C.c_int64 * N_SIZES)(*([-1] * N_SIZES))
        c.dev.ok(c.lib.sh_debug_poison_graph(c.dev.h, KIND[kind], G.h, data_word, index_word(kind, s), sizes))
        with using(c.lib):
            want = owned_bytes(kind, s, len(s.ci) if kind == "frontier" else G.edges)
            assert kind not in ("msf", "match") or G.edges == s.Mw
        if (name, kind) not in _printed:
            _printed.add((name, kind))
            print(f"{what}: bytes poisoned {list(sizes)}")
        assert list(sizes) == want + [0] * (N_SIZES - len(want)), (what, list(sizes), want)
    return before


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_bfs_levels_on_a_poisoned_handle(tools, name):
    starts = S.shape(name).starts
    for i, (word, shares) in enumerate(((ONES, TOP_DOWN), (ZERO, BOTTOM_UP), (ONES, DEFAULT), (ZERO, TOP_DOWN), (ONES, BOTTOM_UP), (ZERO, DEFAULT))):
        bfs(tools, name, starts[i % len(starts)], shares, i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_sssp_on_a_poisoned_handle(tools, name):
    starts, deltas = S.shape(name).starts, sssp_deltas(name)
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        sssp(tools, name, starts[i % len(starts)], deltas[(i // 2) % 2], i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_tri_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        tri(tools, name, ORDERS[i % 2], i != 2, i != 3, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_core_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        core(tools, name, CHASES[(i // 2) % 2], i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_truss_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        truss(tools, name, i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_scc_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        components(tools, name, "scc", SCC_SETTINGS[(i // 2) % 2], i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_wcc_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        components(tools, name, "wcc", SAMPLES[(i // 2) % 2], i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_color_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO, ONES, ZERO)):
        color(tools, name, S.COLOR_SETTINGS[i % 3], i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_msf_on_a_poisoned_handle(tools, name):
    """(ZERO: every best word is a key below every bid of the call, should one survive msf_init)"""
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        msf(tools, name, i < 2, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_match_on_a_poisoned_handle(tools, name):
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        match(tools, name, S.MATCH_SETTINGS[(i // 2) % 2], i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("name", TIER2_NAMES)
def test_rcm_on_a_poisoned_handle(tools, name):
    """(ZERO: every stamp and owner is the smallest word, what an atomic minimum can never lower)"""
    for i, word in enumerate((ONES, ZERO, ONES, ZERO)):
        rcm(tools, name, S.RCM_SETTINGS[(i // 2) % 2], i % 2 == 0, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


@pytest.mark.parametrize("sr", S.FRONTIER_SEMIRINGS, ids=HS.SR_NAME.get)
@pytest.mark.parametrize("name", TIER2_NAMES)
def test_iterate_frontier_on_a_poisoned_handle(tools, name, sr):
    """Sparse launches from launch 2 on, then dense launches only, then sparse ones again, on one handle per plan."""
    for plan in (1, 2):
        for i, (word, share) in enumerate(((ONES, 1.0), (ZERO, 1.0), (ONES, 0.0), (ZERO, 1.0))):
            frontier(tools, name, sr, plan, share, i, S.EXTRA * (i % 2), before=poisoner(tools, name, word))


def test_the_poison_hook_refuses_an_id_outside_the_handle(tools):
    s = S.shape("wheel")
    sizes = (C.c_int64 * N_SIZES)()
    h = tools.handles("wheel")
    F = tools.frontier("wheel", HS.OA, 1)[1]
    for kind, G, bad in (("frontier", F, s.rows), ("bfs", h["bfs"], s.rows), ("sssp", h["sssp"], s.rows), ("scc", h["scc"], s.rows),
                         ("wcc", h["wcc"], s.rows), ("core", h["core"], s.rows), ("truss", h["truss"], s.M),
                         ("color", h["color"], s.rows), ("msf", h["msf"], min(s.rows, s.Mw)), ("match", h["match"], min(s.rows, s.Mw)),
                         ("rcm", h["rcm"], s.rows)):
        assert tools.lib.sh_debug_poison_graph(tools.dev.h, KIND[kind], G.h, ONES, bad, sizes) == abi.SH_EINVAL, kind
    assert tools.lib.sh_debug_poison_graph(tools.dev.h, 12, h["bfs"].h, ONES, 0, sizes) == abi.SH_EINVAL
