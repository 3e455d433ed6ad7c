"""References of sh_bc (betweenness centrality by Brandes' two sweeps) and the graphs its tests share.  Not a test.

Three references, each straight from include/sparseharness_hip.h:
  exact(mat, sources)    the definition in fractions.Fraction: no rounding at all;
  ordered(mat, sources)  the definition in numpy float64 with the header's summation order SUM (list_sum below restates
                         it: pieces of PIECE entries, 64 strided partials, the fixed butterfly, the piece sums left to
                         right), so that the device and the host gold are compared with ==;
  bound(mat, sources)    per vertex the number k of roundings that can feed bc[v].  Each rule adds to the LARGEST count
                         among its operands: a sum of m non-negative terms adds m - 1, a product or a quotient adds 1, a
                         quotient's denominator counts twice, 1 + delta adds 1, each source adds 1.  Every quantity of
                         the recurrences is non-negative, so nothing cancels and |ordered - exact| <= gamma_k * exact
                         with gamma_k = k u / (1 - k u), u = 2^-53.

A matrix is (n, row_ptr, col_idx, val).  Entry (r, c) is the edge c -> r when 0 <= c < n, c != r and the 32 bits of its
value are not all zero; parallel entries are one edge."""
import os
import re
from fractions import Fraction

import numpy as np

LANE, PIECE = 8, 2048     # BC_LANE and BC_PIECE of csrc/bc.hip.h (tests/test_bc_abi.py compares)
BC_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sparseharness_amd", "csrc", "bc.hip.h")
U = Fraction(1, 2 ** 53)
_IDX = np.arange(64)


# ---- graphs
def csr(n, edges, twice=False, reverse=False):
    """(n, rp, ci, va) that stores entry (r, c) for every edge c -> r of `edges` (pairs (c, r)); twice: every entry stored
    twice; reverse: every row's entries in descending column."""
    rows = [[] for _ in range(n)]
    for c, r in edges:
        rows[r].append(c)
    ci, rp = [], [0]
    for r in range(n):
        cs = sorted(rows[r], reverse=reverse)
        if twice:
            cs = [c for c in cs for _ in range(2)]
        ci += cs
        rp.append(len(ci))
    return n, np.array(rp, np.int32), np.array(ci, np.int32), np.ones(len(ci), np.float32)


def restored(mat, twice=False, reverse=False):
    """The same graph stored another way (see csr)."""
    n, rp, ci, va = mat
    keep = (va.view(np.uint32) != 0) & (ci >= 0) & (ci < n)
    r_of = np.repeat(np.arange(n), np.diff(rp))
    return csr(n, list(zip(ci[keep].tolist(), r_of[keep].tolist())), twice=twice, reverse=reverse)


def both(pairs):
    return [e for u, v in pairs for e in ((u, v), (v, u))]


def sym_path(n):
    return csr(n, both((i, i + 1) for i in range(n - 1)))


def star(leaves):
    """Centre 0 and `leaves` leaves, symmetric."""
    return csr(leaves + 1, both((0, 1 + i) for i in range(leaves)))


def cycle(n):
    return csr(n, [(i, (i + 1) % n) for i in range(n)])


def diamonds(k, middles):
    """A directed chain of k diamonds: a_i -> each of `middles` vertices -> a_{i+1}; a_i = i * (middles + 1).  sigma(a_k) =
    middles^k from a_0."""
    step = middles + 1
    edges = []
    for i in range(k):
        a, b = i * step, (i + 1) * step
        for j in range(middles):
            edges += [(a, a + 1 + j), (a + 1 + j, b)]
    return csr(k * step + 1, edges)


def bipartite(p, q):
    return csr(p + q, both((i, p + j) for i in range(p) for j in range(q)))


def two_levels(width):
    """0 -> 1 .. width (symmetric), and a last vertex joined to all of them: one level wider than a launch has lanes."""
    n = width + 2
    mid = np.arange(1, width + 1, dtype=np.int32)
    ends = np.stack([np.zeros(width, np.int32), np.full(width, n - 1, np.int32)], axis=1).ravel()
    ci = np.concatenate([mid, ends, mid])
    rp = np.concatenate([[0], width + 2 * np.arange(width + 1), [4 * width]]).astype(np.int32)
    return n, rp, ci, np.ones(len(ci), np.float32)


def digraph4(A):
    """One graph of small_graphs_ref.all_digraphs(4, loops=False): A[r, c] is a stored entry of row r, the edge c -> r."""
    return csr(4, [(c, r) for r in range(4) for c in range(4) if A[r, c]])


def graphs4(pick=None):
    """The digraphs on 4 vertices (small_graphs_ref.all_digraphs without loops: 4096 of them; pick: the indices of a
    selection, None for all) side by side in one matrix, graph i of the selection on the vertices 4i .. 4i + 3."""
    import small_graphs_ref as S
    A = S.all_digraphs(4, loops=False)
    if pick is not None:
        A = A[np.asarray(pick)]
    g, r, c = np.nonzero(A)
    n = 4 * len(A)
    key = np.unique((4 * g + r) * n + 4 * g + c)
    rp = np.searchsorted(key // n, np.arange(n + 1)).astype(np.int32)
    return n, rp, (key % n).astype(np.int32), np.ones(len(key), np.float32)


def with_values(rp, ci):
    return len(rp) - 1, rp, ci, np.ones(len(ci), np.float32)


def lists(mat, duplicates=False):
    """-> (ins, outs): per vertex the ascending array of its in-neighbours and of its out-neighbours."""
    n, rp, ci, va = mat
    r_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    c = ci.astype(np.int64)
    keep = (np.ascontiguousarray(va).view(np.uint32) != 0) & (c >= 0) & (c < n) & (c != r_of)
    key = r_of[keep] * n + c[keep]
    key = np.sort(key) if duplicates else np.unique(key)
    r, c = key // n, key % n
    ins = np.split(c, np.searchsorted(r, np.arange(1, n)))
    o = np.lexsort((r, c))
    outs = np.split(r[o], np.searchsorted(c[o], np.arange(1, n)))
    return ins, outs


# ---- the header's SUM
def list_sum(t):
    """SUM of the terms t[0 .. len) of a list (float64; +0.0 where an entry does not take part)."""
    t = np.asarray(t, np.float64)
    acc = np.float64(0.0)
    for p0 in range(0, len(t), PIECE):
        piece = t[p0:p0 + PIECE]
        rows = np.concatenate([piece, np.zeros(-len(piece) % 64)]).reshape(-1, 64)   # (x + 0.0 == x: the padding is exact)
        partial = np.zeros(64)
        for row in rows:
            partial = partial + row
        for o in (32, 16, 8, 4, 2, 1):
            partial = partial + partial[_IDX ^ o]
        acc = acc + partial[0]
    return acc


def left_to_right(t):
    acc = np.float64(0.0)
    for x in np.asarray(t, np.float64):
        acc = acc + x
    return acc


def _sweep(ins, outs, n, s):
    """-> (level, levels): the BFS levels from s."""
    level = np.full(n, -1, np.int32)
    level[s] = 0
    levels = [np.array([s], np.int64)]
    while True:
        near = np.concatenate([outs[v] for v in levels[-1]]) if len(levels[-1]) else np.zeros(0, np.int64)
        new = np.unique(near[level[near] < 0])
        if len(new) == 0:
            return level, levels
        level[new] = len(levels)
        levels.append(new)


def ordered(mat, sources, bc=None, mutant=None):
    """-> dict(bc, sigma, level, depth, reached, sigma_max, edges) in the header's arithmetic.  bc: scores to add to
    (accumulate = 1).  mutant: "order" sums left to right, "duplicates" lets stored duplicates count, "source" counts the
    source too -- what tests/test_bc_ref.py shows the references to notice."""
    n = mat[0]
    ins, outs = lists(mat, duplicates=mutant == "duplicates")
    total = left_to_right if mutant == "order" else list_sum
    bc = np.zeros(n) if bc is None else np.array(bc, np.float64)
    sigma, level = np.zeros(n), np.full(n, -1, np.int32)
    depth, reached, smax, walked = [], [], [], []
    with np.errstate(all="ignore"):
        for s in sources:
            level, levels = _sweep(ins, outs, n, s)
            sigma, delta = np.zeros(n), np.zeros(n)
            sigma[s] = 1.0
            for L in range(1, len(levels)):
                for w in levels[L]:
                    v = ins[w]
                    sigma[w] = total(np.where(level[v] == L - 1, sigma[v], 0.0))
            for L in range(len(levels) - 2, -1 if mutant == "source" else 0, -1):
                for v in levels[L]:
                    w = outs[v]
                    delta[v] = total(np.where(level[w] == L + 1, (sigma[v] / sigma[w]) * (1.0 + delta[w]), 0.0))
                    bc[v] = bc[v] + delta[v]
            depth.append(len(levels) - 1)
            reached.append(sum(len(x) for x in levels))
            smax.append(sigma.max() if n else 0.0)
            walked.append(sum(len(outs[v]) for x in levels for v in x))
    return dict(bc=bc, sigma=sigma, level=level, depth=np.array(depth, np.int32), reached=np.array(reached, np.int64),
                sigma_max=np.array(smax, np.float64), edges=np.array(walked, np.int64))


def exact(mat, sources):
    """-> bc as a list of Fractions, straight from the definition."""
    n = mat[0]
    ins, outs = lists(mat)
    bc = [Fraction(0)] * n
    for s in sources:
        level, levels = _sweep(ins, outs, n, s)
        sigma, delta = [Fraction(0)] * n, [Fraction(0)] * n
        sigma[s] = Fraction(1)
        for L in range(1, len(levels)):
            for w in levels[L]:
                sigma[w] = sum((sigma[v] for v in ins[w] if level[v] == L - 1), Fraction(0))
        for L in range(len(levels) - 2, -1, -1):
            for v in levels[L]:
                delta[v] = sum((sigma[v] / sigma[w] * (1 + delta[w]) for w in outs[v] if level[w] == L + 1), Fraction(0))
                if v != s:
                    bc[v] += delta[v]
    return bc


def bound(mat, sources):
    """-> k[v]: the roundings that can feed bc[v] (see the module's docstring for the rules)."""
    n = mat[0]
    ins, outs = lists(mat)
    kb = [0] * n
    for s in sources:
        level, levels = _sweep(ins, outs, n, s)
        ks, kd = [0] * n, [0] * n
        for L in range(1, len(levels)):
            for w in levels[L]:
                part = [ks[v] for v in ins[w] if level[v] == L - 1]
                ks[w] = max(part) + len(part) - 1
        for L in range(len(levels) - 2, 0, -1):
            for v in levels[L]:
                part = [max(max(ks[v], 2 * ks[w]) + 1, kd[w] + 1) + 1 for w in outs[v] if level[w] == L + 1]
                kd[v] = max(part) + len(part) - 1 if part else 0
                kb[v] = max(kb[v], kd[v]) + 1
    return kb


def gamma(k):
    return k * U / (1 - k * U)


# ---- what the kernel file states, and the cases the device is compared on
def constants():
    """-> the `constexpr int BC_...` of csrc/bc.hip.h by name."""
    return {k: int(v) for k, v in re.findall(r"constexpr int (BC_\w+) = (\d+);", open(BC_HEADER).read())}


def header_footprint(n, edges):
    """The formula of include/sparseharness_hip.h (tests/test_bc_abi.py parses the header's and compares)."""
    return 12 * (n + 1) + 24 * n + 8 * edges + 16 * (edges // 1024 + 1) + 17408


def star_sizes():
    """Leaves either side of the tiers of the list sum and of a wave's stride."""
    c = constants()
    lane, piece = c["BC_LANE"], c["BC_PIECE"]
    return (lane - 1, lane, lane + 1, 63, 64, 65, piece - 1, piece, piece + 1, 2 * piece + 1)


def wide():
    """A level wider than a launch has lanes."""
    return constants()["BC_MAX_BLOCKS"] * 256 + 77


def _edges():
    import graph_patterns as P
    return with_values(*P.edges_pattern())


def _rmat10():
    from sparseharness_amd import hostlib as H
    return (1 << 10,) + H.rmat(10, seed=40)


# name -> (matrix, sources, reference: "ordered" | "host"); "host": the shapes Python cannot afford
CASES = {
    "graphs4": (graphs4, lambda n: list(range(n)), "host"),   # all 4096 digraphs, every vertex a source
    "path100": (lambda: sym_path(100), lambda n: list(range(n)), "ordered"),
    "star65-all": (lambda: star(65), lambda n: list(range(n)), "ordered"),
    "cycle37": (lambda: cycle(37), lambda n: list(range(n)), "ordered"),
    "diamonds33": (lambda: diamonds(33, 3), lambda n: [0], "ordered"),
    "diamonds34": (lambda: diamonds(34, 3), lambda n: [0], "ordered"),
    "diamonds1030": (lambda: diamonds(1030, 2), lambda n: [0], "ordered"),
    "K7,9": (lambda: bipartite(7, 9), lambda n: list(range(n)), "ordered"),
    "edges0": (_edges, lambda n: [0], "ordered"),
    "edges8192": (_edges, lambda n: [8192], "ordered"),
    "rmat10": (_rmat10, lambda n: np.random.default_rng(5).integers(0, n, 16).tolist(), "ordered"),
    "two-levels": (lambda: two_levels(wide()), lambda n: [0, 1, n - 1], "host"),
    "path300": (lambda: sym_path(300), lambda n: [0], "ordered"),
    "dead-end": (lambda: csr(5, [(0, 1), (1, 2), (3, 4)]), lambda n: [2, 0, 4], "ordered"),
}
CASES.update({f"star{k}": (lambda k=k: star(k), lambda n: [1, 0, 2], "ordered") for k in star_sizes()})
_cache, _want = {}, {}


def case(name):
    """-> (matrix, sources), made once."""
    if name not in _cache:
        make, sources, _ = CASES[name]
        mat = make()
        _cache[name] = (mat, [int(s) for s in sources(mat[0])])
    return _cache[name]


def want(name):
    """The reference's answer for a case, computed once and left unchanged."""
    if name not in _want:
        mat, sources = case(name)
        if CASES[name][2] == "host":
            from sparseharness_amd import hostlib as H
            bc, sigma, level, depth, reached, smax, edges = H.bc_scores(*mat[1:], sources)
            r = dict(bc=bc, sigma=sigma, level=level, depth=depth, reached=reached, sigma_max=smax, edges=edges)
        else:
            r = ordered(mat, sources)
        for v in r.values():
            v.setflags(write=False)
        _want[name] = r
    return _want[name]
