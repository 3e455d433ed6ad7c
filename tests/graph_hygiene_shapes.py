"""Inputs and references for the graph-hygiene tests: what a graph or worklist call may read is its operands and its
handle, what it may write is `rows` (`edges`) elements of its outputs.  CPU only: numpy, the references the suite already
pins (small_graphs_ref for the unions, and rcm_ref.levels for sh_rcm, which has no tensor form; oracle_bfs, sssp_ref,
scc_ref, wcc_ref, tri_ref, core_ref, truss_ref, color_ref, msf_ref, match_ref, rcm_ref for the wheel; the C oracle's iterate
for sh_iterate_frontier); nothing here touches the engine.  Not a test and not a conftest.
tests/test_graph_hygiene_cpu.py asserts on these references that a word written one element too far, left unwritten or read
from a guard would show; tests/test_graph_hygiene_gpu.py runs the engine on them.

Shapes, the smallest that leave every boundary of the kernels (64 rows per wave step, 32 rows per bitmap word, 256 rows
per workgroup, pieces of 2048 / 4096 list entries):
  odd unions: the disjoint union of G' of the 1024 simple graphs on 5 vertices (rows = 5 G' = 65, 95, 225, 255, 5115) and
      of 181 of the 512 digraphs with loops on 3 vertices (rows = 543), each under both numberings of small_graphs_ref.
      Each subset is one window of the enumeration chosen to hold dense graphs (the last element of every output is then
      not what an initialisation leaves), a graph with an isolated vertex (one vertex at least is unreached) and a graph
      that is searched two levels deep.
  the wheel: n = 4131 vertices, the rim a cycle 0 .. n - 2, the hub n - 1 joined to every rim vertex: the hub's list of
      4130 entries goes through the piece paths of every handle, its output element is the last word before the guard,
      its bit lies in the partial last bitmap word (n % 32 = 3), and the last edge id (M = 8260) is the hub's.  Rim edges
      weigh 1, spokes 0.5: every float32 path sum is exact.  Searched from one rim vertex and, in a second case, from the
      hub.

Guard words of the inputs mean something if they are read: 1 behind x0 of sh_bfs_levels (a source), 0x00000000 behind x0
of sh_sssp (a source at distance 0, and what fresh memory holds), hygiene_shapes.POISON[sr] around x, y0 and scratch of
sh_iterate_frontier, 0x7FFFFFFF around prio of sh_color (a priority above every vertex's).  sh_msf and sh_match read
weights: small_graphs_ref.weights on the unions (asymmetric pairs, ties, -1.5, -0.0, +inf, a NaN, one stored +0.0), rim
1 and spokes 0.5 on the wheel.  Outputs are prefilled with 0xDEADBEEF and sit between guards of it."""
import functools

import numpy as np

import bfs_ref
import color_ref
import core_ref
import hygiene_shapes as HS
import match_ref
import msf_ref
import rcm_ref
import scc_ref
import small_graphs_ref as R
import sssp_ref
import tri_ref
import truss_ref
import wcc_ref
from oracle import oracle as O

DEAD = 0xDEADBEEF
BFS_X0_GUARD, SSSP_X0_GUARD = 1, 0x00000000
EXTRA = 3                         # elements behind `rows` that a call must leave alone
FLT_MAX = R.FLT_MAX

# name -> (kind, n, first graph, graphs): a window of the enumeration (high indices have more bits set: denser graphs)
WINDOWS = {"u5x13": ("undirected", 5, 1007, 13), "u5x19": ("undirected", 5, 1004, 19), "u5x45": ("undirected", 5, 979, 45),
           "u5x51": ("undirected", 5, 973, 51), "u5x1023": ("undirected", 5, 1, 1023), "d3x181": ("digraphs", 3, 331, 181)}
RESIDUES = {"u5x13": (65, 1, 1, 65), "u5x19": (95, 31, 31, 95), "u5x45": (225, 1, 33, 225), "u5x51": (255, 31, 63, 255),
            "u5x1023": (5115, 27, 59, 251), "d3x181": (543, 31, 31, 31)}   # rows, rows % 32, % 64, % 256
UNION_NAMES = tuple(f"{w}-{numbering}" for w in WINDOWS for numbering in R.NUMBERINGS)
WHEEL_N = 4131
WHEEL_M = 2 * (WHEEL_N - 1)
WHEEL_RIM_SOURCE = 1000
NAMES = UNION_NAMES + ("wheel",)
FRONTIER_NAMES = ("u5x51-blocks", "wheel")   # the shapes sh_iterate_frontier runs on
DELTA, FRONTIER_CAP = 1e-4, 64
# the settings sh_color, sh_match and sh_rcm run under here.  Order 0 and the prio vector put the wheel's hub last, so
# that its colour, the last word before the guard, is 2 at least; order 2 puts it first.
COLOR_SETTINGS = ((0, 0, False), (2, 1, False), (1, 1, True))   # (order, seed, prio)
MATCH_SETTINGS = ((1, 1), (0, 0))                               # (heavy, seed)
RCM_SETTINGS = ((8, 1), (0, 0))                                 # (sweeps, reverse)
PRIO_GUARD = 0x7FFFFFFF   # around prio: a priority above every vertex's, so that a guard read as a priority shows


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


class Start:
    """One set of sources: x0 of sh_bfs_levels (int32 0 / 1) and of sh_sssp (float32) with the answers."""

    def __init__(self, label, sources, x0, bfs, sssp, bfs_cut=None):
        self.label, self.sources, self.x0, self.bfs, self.sssp, self.bfs_cut = label, sources, x0, frozen(bfs), frozen(sssp), bfs_cut
        for a in (sources, x0):
            a.setflags(write=False)


class Shape:
    """rp / ci / val: the pattern as bfs, sssp and scc get it (val: the weights of sssp; bfs and scc get ones);
    rp1 / ci1: as wcc, tri, core, truss, color and rcm get it (the undirected shapes stored one way); rp / ci / wval: as
    msf and match get it (the unions: small_graphs_ref.weights; the wheel: val), Mw its edges (a stored +0.0 is no entry);
    prio: the priority vector of sh_color.  want[entry point]: dict of the expected vectors and scalars -- for color, match
    and rcm one dict per setting; cut (the wheel): the same after max_rounds = 1 / max_steps = 1; starts: the source sets."""


def _components(comp):
    return int(np.count_nonzero(comp == np.arange(len(comp))))


@functools.lru_cache(maxsize=None)
def shape(name):
    return wheel() if name == "wheel" else union(*name.split("-"))


def union(window, numbering):
    kind, n, first, graphs = WINDOWS[window]
    A = (R.all_digraphs(n) if kind == "digraphs" else R.all_undirected(n))[first:first + graphs]
    s = Shape()
    s.name, s.kind, s.numbering, s.A, s.rows = f"{window}-{numbering}", kind, numbering, A, graphs * n
    s.rp, s.ci, (g, r, c) = R.union(A, numbering)
    val, x0, src = R.sssp_inputs(graphs, n)
    s.val = np.ascontiguousarray(val[g, r, c])
    s.rp1, s.ci1 = (s.rp, s.ci) if kind == "digraphs" else R.union(A, numbering, R.halves(A))[:2]
    b, d, t, c_, k = R.bfs(A, src), R.sssp(A, val, x0), R.triangles(A), R.core(A), R.truss(A, numbering)
    s.M, s.local = k["M"], dict(src=src, val=val, x0=x0)
    s.starts = (Start("", R.scatter(src.astype(np.int32), numbering), R.scatter(x0, numbering),
                      dict(level=R.scatter(b["level"], numbering).astype(np.int32), parent=R.to_global(b["parent"], numbering).astype(np.int32),
                           depth=b["depth"], reached=b["reached"], complete=True, sizes=b["sizes"]),
                      dict(dist=R.bits(R.scatter(d["dist"], numbering)), pred=R.to_global(d["pred"], numbering).astype(np.int32),
                           reached=d["reached"], complete=True)),)
    scc, wcc = (R.to_global(f(A), numbering).astype(np.int32) for f in (R.scc, R.wcc))
    deg = R.scatter(t["deg"], numbering).astype(np.int32)
    s.want = dict(scc=dict(comp=scc, components=_components(scc)), wcc=dict(comp=wcc, components=_components(wcc)),
                  tri=dict(tri=R.scatter(t["tri"], numbering).astype(np.uint64), deg=deg, triangles=t["total"]),
                  core=dict(core=R.scatter(c_["core"], numbering).astype(np.int32), deg=deg, degeneracy=c_["degeneracy"]),
                  truss=dict(truss=k["truss"], support=k["support"], edge_u=k["edge_u"], edge_v=k["edge_v"],
                             max_truss=k["max_truss"], triangles=k["triangles"], edges=k["M"]))
    wv, prio = R.weights(graphs, n), R.prio_of(graphs, n)
    s.wval, s.prio = np.ascontiguousarray(wv[g, r, c]), R.scatter(prio, numbering).astype(np.int32)
    f = R.msf(A, wv, numbering)
    s.Mw = f["M"]
    edge = lambda d: dict(edge_u=d["edge_u"], edge_v=d["edge_v"], weight=d["weight"])   # noqa: E731
    s.want["msf"] = dict(in_msf=f["in_msf"], comp=R.to_global(f["comp"], numbering).astype(np.int32), tree_edges=f["tree_edges"],
                         components=f["components"], **edge(f))
    s.want["color"], s.want["match"], s.want["rcm"] = {}, {}, {}
    for order, seed, with_prio in COLOR_SETTINGS:
        c = R.coloring(A, R.color_keys(A, numbering, order, seed, prio if with_prio else None))
        s.want["color"][(order, seed, with_prio)] = dict(color=R.scatter(c["color"], numbering).astype(np.int32), colors=c["colors"],
                                                         rounds=int(c["depth"].max()) + 1)
    for heavy, seed in MATCH_SETTINGS:
        m = R.matching(A, wv, numbering, heavy, seed)
        s.want["match"][(heavy, seed)] = dict(mate=R.to_global(m["mate"], numbering).astype(np.int32), in_match=m["in_match"],
                                              pairs=m["pairs"], **edge(m))
    for sweeps, reverse in RCM_SETTINGS:
        s.want["rcm"][(sweeps, reverse)] = _rcm(s, sweeps, reverse)
    _freeze_all(s.want)
    return s


RCM_SCALARS = ("components", "sweeps_run", "steps", "complete", "bandwidth_before", "bandwidth_after", "profile_before", "profile_after")


def _rcm(s, sweeps, reverse, max_steps=None):
    """rcm_ref.levels on the shape as one matrix: sh_rcm has no tensor form, and the walk in (deg, index) orders the
    components of a union."""
    w = rcm_ref.levels(s.rows, s.rp1, s.ci1, np.ones(len(s.ci1), np.float32), sweeps=sweeps, reverse=reverse, max_steps=max_steps)
    return {k: w[k] for k in ("perm", "pos", "level", "kind", "size", "edges") + RCM_SCALARS}


def _freeze_all(want):
    for d_ in want.values():
        frozen(d_)
        for inner in d_.values():
            if isinstance(inner, dict):
                frozen(inner)


def _four_on_the_wheel(s, max_rounds=None):
    """color_ref, msf_ref, match_ref and rcm_ref on the wheel; max_rounds = 1: what a run cut short after one round (one
    step) leaves, by the references' own max_rounds / max_steps forms."""
    n, ones1 = s.rows, np.ones(len(s.ci1), np.float32)
    want = dict(color={}, match={}, rcm={})
    for order, seed, with_prio in COLOR_SETTINGS:
        c = color_ref.schedule(n, s.rp1, s.ci1, ones1, order=order, seed=seed, prio=s.prio if with_prio else None, max_rounds=max_rounds)
        want["color"][(order, seed, with_prio)] = dict(color=c["color"], colors=c["colors"], rounds=c["rounds"], complete=c["complete"],
                                                       coloured=c["coloured"])
    f = msf_ref.schedule(n, s.rp, s.ci, s.wval, **({} if max_rounds is None else dict(max_rounds=max_rounds)))
    want["msf"] = dict(in_msf=f["in_msf"], comp=f["comp"], edge_u=f["eu"], edge_v=f["ev"], weight=f["weight"], tree_edges=f["tree_edges"],
                       components=f["components"], complete=f["complete"])
    for heavy, seed in MATCH_SETTINGS:
        m = match_ref.rounds(n, f["eu"], f["ev"], match_ref.mkeys(msf_ref.order_key(f["weight"]), heavy, seed),
                             **({} if max_rounds is None else dict(max_rounds=max_rounds)))
        want["match"][(heavy, seed)] = dict(mate=m["mate"], in_match=m["in_match"], pairs=m["pairs"], complete=m["complete"],
                                            edge_u=f["eu"], edge_v=f["ev"], weight=f["weight"])
    for sweeps, reverse in RCM_SETTINGS:
        want["rcm"][(sweeps, reverse)] = _rcm(s, sweeps, reverse, max_steps=max_rounds)
    _freeze_all(want)
    return want, f["M"]


def wheel():
    n, hub = WHEEL_N, WHEEL_N - 1
    rim = np.arange(n - 1, dtype=np.int64)
    a, b = np.concatenate([rim, rim]), np.concatenate([(rim + 1) % (n - 1), np.full(n - 1, hub)])
    s = Shape()
    s.name, s.kind, s.numbering, s.rows, s.M = "wheel", "wheel", None, n, WHEEL_M
    _, s.rp, s.ci, _ = tri_ref.from_pairs(n, a, b)                  # both ways
    _, s.rp1, s.ci1, _ = tri_ref.from_pairs(n, a, b, both=False)    # one way, in the row of the second end: the hub's row holds every spoke
    row = np.repeat(np.arange(n), np.diff(s.rp))
    s.val = np.where((row == hub) | (s.ci == hub), np.float32(0.5), np.float32(1.0)).astype(np.float32)
    ones, ones1 = np.ones(len(s.ci), np.float32), np.ones(len(s.ci1), np.float32)
    starts = []
    for label, v in (("rim", WHEEL_RIM_SOURCE), ("hub", hub)):
        src = np.zeros(n, np.int32)
        src[v] = 1
        x0 = np.where(src != 0, np.float32(0), FLT_MAX).astype(np.float32)
        o, cut = bfs_ref.oracle_bfs(n, s.rp, s.ci, ones, src), bfs_ref.oracle_bfs(n, s.rp, s.ci, ones, src, max_levels=1)
        dist, pred, reached, _ = sssp_ref.sssp(s.rp, s.ci, s.val, x0)
        as_dict = lambda o: dict(level=o.level, parent=o.parent, depth=o.depth, reached=o.reached, complete=o.complete, sizes=o.sizes)   # noqa: E731
        starts.append(Start(label, src, x0, as_dict(o), dict(dist=R.bits(dist), pred=pred, reached=reached, complete=True),
                            frozen(as_dict(cut))))
    s.starts = tuple(starts)
    scc, wcc = scc_ref.components(n, s.rp, s.ci, ones), wcc_ref.components(n, s.rp1, s.ci1, ones1)
    tri, deg, m = tri_ref.counts(n, s.rp1, s.ci1, ones1)
    c_, k = core_ref.peel(n, s.rp1, s.ci1, ones1), truss_ref.peel(n, s.rp1, s.ci1, ones1)
    assert m == c_["M"] == k["M"] == WHEEL_M
    s.want = dict(scc=dict(comp=scc, components=_components(scc)), wcc=dict(comp=wcc, components=_components(wcc)),
                  tri=dict(tri=tri, deg=deg, triangles=int(tri.sum()) // 3),
                  core=dict(core=c_["core"], deg=c_["deg"], degeneracy=c_["degeneracy"]),
                  truss=dict(truss=k["truss"], support=k["support"], edge_u=k["edge_u"], edge_v=k["edge_v"],
                             max_truss=k["max_truss"], triangles=k["triangles"], edges=k["M"]))
    s.wval = s.val
    s.prio = (np.arange(n) % 3).astype(np.int32)
    s.prio[hub] = -1   # the hub last
    four, s.Mw = _four_on_the_wheel(s)
    s.want.update(four)
    s.cut, _ = _four_on_the_wheel(s, max_rounds=1)
    assert s.Mw == WHEEL_M
    _freeze_all(s.want)
    return s


# ------------------------------------------------------------------ sh_iterate_frontier: the three semirings it serves
FRONTIER_SEMIRINGS = (HS.MP, HS.OA, HS.MM)
FRONTIER_SCALARS = HS.LOOP_SCALARS


@functools.lru_cache(maxsize=None)
def frontier_case(name, sr):
    """-> (values, x0, want, launches, converged): the shape's pattern (both ways) under the semiring, started from the
    first source set with y0 = x0, by the oracle's iterate."""
    s = shape(name)
    src = s.starts[0].sources != 0
    if sr == HS.MP:
        va, x0 = np.abs(s.val), np.minimum(np.abs(s.starts[0].x0), FLT_MAX)
    elif sr == HS.OA:
        va, x0 = np.ones(len(s.ci), np.int32), src.astype(np.int32)
    else:   # the largest label, at the sources, runs down the graph
        va, x0 = np.full(len(s.ci), 1 << 20, np.int32), np.where(src, 1000, -1).astype(np.int32)
    want, launches, converged = O.iterate(sr, s.rp, s.ci, va, x0, x0, *FRONTIER_SCALARS[sr], DELTA, FRONTIER_CAP)
    for a in (va, x0, want):
        a.setflags(write=False)
    return va, x0, want, launches, bool(converged)
