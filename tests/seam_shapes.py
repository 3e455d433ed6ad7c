"""Inputs whose run-ahead loops end exactly where a batch of gated launches ends, one launch before and one after; and the
references of those runs, computed once and shared.  CPU only: numpy, the C oracle and the numpy references of the other
test modules; nothing here touches the engine.  Not a test and not a conftest.  tests/test_seams_cpu.py proves from the
references alone that every input hits the count it is built for; tests/test_seams_gpu.py runs the engine on them.

sh_iterate, sh_iterate_multi, sh_bits_iterate and sh_iterate_frontier (under dense_share = 0) enqueue 8 launches at a
time: their seams lie at launches 8, 16, 24.  run_batches (sh_bfs_levels, sh_sssp, sh_scc, sh_wcc, sh_core, sh_truss)
grows its batches 8, 16, 32, 32: its seams lie at steps 8, 24, 56, 88.

comb(n, hub): vertices 0 .. n - 1 are a directed path (row i + 1 stores column i), then `hub` leaves with empty rows, then
one hub vertex whose row reads column n - 1 and every leaf: hub + 1 entries, above the CSR-stream plan's long-row
threshold (4096) and heavy for the tiled plan, so the fix-up kernels run, gated, in every launch.  A mark started at
path vertex s walks to n - 1 in n - 1 - s launches, reaches the hub one launch later and is confirmed by one more:
n - s + 1 launches for (or,and) with alpha = beta = 1 and for (min,+) with alpha = beta = 0; started at the hub it is 1.
(+,x) with alpha = 1, beta = 0 moves the mark instead of keeping it, and the zero vector that follows the hub needs a
launch of its own: n - s + 2, 2 from the hub, 1 from the zero vector.  (max,min) with alpha = beta = 2^30, values 2^20
and x0 = n - 1, ..., 0 down the path (leaves -1, hub -2) lets the largest label run down the path and into the hub; the
number of path vertices for a given count is looked up with the oracle (maxmin_path_len), and count 1 starts from the
fixed point.
"""
import functools

import numpy as np

import core_ref
import scc_ref
import sssp_ref
import test_bfs_levels_gpu as BL
import tri_ref as T
import truss_ref
import wcc_ref as W
from oracle import oracle as O

S8 = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25)                              # batches of 8
S32 = (1, 7, 8, 9, 23, 24, 25, 55, 56, 57, 87, 88, 89)                # run_batches: seams at 8, 24, 56, 88
S32_TRUSS = tuple(r for r in S32 if r <= 57)                          # (the Python truss reference takes 2 s at 57 rounds)

PT, MP, OA, MM = O.PLUS_TIMES_F32, O.MIN_PLUS_F32, O.OR_AND_I32, O.MAX_MIN_I32
SR_NAME = {PT: "plus_times", MP: "min_plus", OA: "or_and", MM: "max_min"}
SCALARS = {PT: (1.0, 0.0), MP: (0.0, 0.0), OA: (1, 1), MM: (1 << 30, 1 << 30)}
VALUE = {PT: 1.0, MP: 1.0, OA: 1, MM: 1 << 20}
DELTA = 1e-4
N_PATH, HUB = 24, 5000            # the comb of the three semirings with a source: counts 1 .. 25 (26 for (+,x))
UNCAPPED = 1000                   # a launch cap no run here comes near


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------ the comb
@functools.lru_cache(maxsize=None)
def comb(n, hub=HUB):
    """-> (N, rp, ci): N = n + hub + 1 vertices, the hub vertex is N - 1."""
    N = n + hub + 1
    deg = np.zeros(N, np.int64)
    deg[1:n] = 1
    deg[N - 1] = hub + (1 if n else 0)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = np.concatenate([np.arange(0, max(n - 1, 0)), [n - 1] if n else [], np.arange(n, n + hub)]).astype(np.int32)
    assert len(ci) == rp[-1]
    return (N,) + frozen(rp, ci)


def values(sr, nnz):
    return np.full(nnz, VALUE[sr], O.elem_dtype(sr))


def one_hot(sr, N, v):
    """The start vector of a single source v (None: no source at all)."""
    x = np.full(N, O.FLT_MAX, np.float32) if sr == MP else np.zeros(N, O.elem_dtype(sr))
    if v is not None:
        x[v] = 0.0 if sr == MP else 1
    return x


def source_for(sr, L, n=N_PATH, hub=HUB):
    """The vertex of comb(n, hub) from which semiring sr takes exactly L launches (None: the zero vector)."""
    hub_vertex = n + hub
    if sr == PT:
        if L <= 2:
            return (None, hub_vertex)[L - 1]
        s = n + 2 - L
    else:
        if L == 1:
            return hub_vertex
        s = n + 1 - L
    assert 0 <= s < n, (sr, L)
    return s


@functools.lru_cache(maxsize=None)
def maxmin_start(n, hub=HUB):
    N = n + hub + 1
    x0 = np.full(N, -1, np.int32)
    x0[:n] = np.arange(n - 1, -1, -1)
    x0[N - 1] = -2
    return frozen(x0)[0]


@functools.lru_cache(maxsize=None)
def maxmin_path_len(L):
    """The number of path vertices with which the (max,min) comb takes exactly L launches (L >= 2), by the oracle."""
    a, b = SCALARS[MM]
    for n in range(1, L + 2):
        N, rp, ci = comb(n)
        x0 = maxmin_start(n)
        if O.iterate(MM, rp, ci, values(MM, len(ci)), x0, x0, a, b, DELTA, UNCAPPED)[1:] == (L, True):
            return n
    raise AssertionError(f"no (max,min) comb takes {L} launches")


@functools.lru_cache(maxsize=None)
def iterate_case(sr, L):
    """-> dict(N, rp, ci, va, x0, alpha, beta) of the single-source run of L launches; y0 = x0."""
    if sr == MM:
        n = 2 if L == 1 else maxmin_path_len(L)
        N, rp, ci = comb(n)
        va = values(sr, len(ci))
        x0 = maxmin_start(n)
        if L == 1:   # the fixed point of the ordinary start: one launch confirms it
            x0 = frozen(O.iterate(MM, rp, ci, va, x0, x0, *SCALARS[MM], DELTA, UNCAPPED)[0])[0]
    else:
        N, rp, ci = comb(N_PATH)
        va = values(sr, len(ci))
        x0 = frozen(one_hot(sr, N, source_for(sr, L)))[0]
    return dict(N=N, rp=rp, ci=ci, va=frozen(va)[0], x0=x0, alpha=SCALARS[sr][0], beta=SCALARS[sr][1], n_path=N - HUB - 1)


@functools.lru_cache(maxsize=None)
def iterate_ref(sr, L, cap=UNCAPPED):
    """O.iterate on iterate_case(sr, L) stopped at `cap` -> (vector, launches, converged)."""
    c = iterate_case(sr, L)
    x, it, conv = O.iterate(sr, c["rp"], c["ci"], c["va"], c["x0"], c["x0"], c["alpha"], c["beta"], DELTA, cap)
    return frozen(x)[0], it, conv


def caps_for(L):
    """The caps of a run of L launches, in the order they are applied to one uploaded matrix."""
    return [c for c in (L - 1, L, L + 1) if c >= 1]


@functools.lru_cache(maxsize=None)
def iterates(sr, L, launches):
    """x_0 .. x_launches of iterate_case(sr, L) by O.kernel, one launch at a time."""
    c = iterate_case(sr, L)
    xs = [c["x0"]]
    for _ in range(launches):
        xs.append(frozen(O.kernel(sr, c["rp"], c["ci"], c["va"], xs[-1], xs[-1], c["alpha"], c["beta"]))[0])
    return tuple(xs)


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frontier_modes(sr, L, launches, share):
    """mode_per_iter by the header's rule: launches 0 and 1 dense; launch k >= 2 sparse when the transposed columns of
    the rows that launch k - 1 changed hold at most dense_share * nnz entries (uint32 of the product, as the engine
    takes it); dense_share 0: never; >= 1: always."""
    c = iterate_case(sr, L)
    N, ci = c["N"], c["ci"]
    col_len = np.bincount(ci[(ci >= 0) & (ci < N)], minlength=N)
    xs = iterates(sr, L, launches)
    limit = None if share >= 1.0 else int(share * float(len(ci)))
    modes = []
    for k in range(launches):
        if k < 2 or share == 0.0:
            modes.append(0)
            continue
        changed = bits_of(xs[k]) != bits_of(xs[k - 1])
        modes.append(1 if limit is None or int(col_len[changed].sum()) <= limit else 0)
    return modes


def frontier_changed(sr, L, launches):
    xs = iterates(sr, L, launches)
    return [int((bits_of(xs[k + 1]) != bits_of(xs[k])).sum()) for k in range(launches)]


# ------------------------------------------------------------------ several sources at once
COUNTS4 = ((1, 8, 9, 16), (1, 9, 17, 25))                 # width 4: two placements; 8, 9, 16 and 17 are all hit
COUNTS32 = tuple(S8[(7 * j) % len(S8)] for j in range(32))  # every value of S8, neighbours in different batches


def counts_of_sources(n_src):
    """The launch count wanted of each of n_src sources (n_src a multiple of 32): COUNTS32's cycle, so that every
    32-bit word of a packed vector holds sources of every count."""
    return tuple(S8[(7 * s) % len(S8)] for s in range(n_src))


@functools.lru_cache(maxsize=None)
def source_ref(sr, L, cap=UNCAPPED):
    """The single-source reference of the column that is to take L launches, stopped at cap."""
    return iterate_ref(sr, L, cap)


def multi_caps(counts):
    """Every distinct column count and that count - 1."""
    return sorted({c for L in set(counts) for c in (L - 1, L) if c >= 1})


@functools.lru_cache(maxsize=None)
def level_sizes(L, launches):
    """newly_set of one (or,and) source that takes L launches: vertices switched on by launch l, for l < launches."""
    xs = iterates(OA, L, launches)
    return tuple(int(((xs[k] == 0) & (xs[k + 1] != 0)).sum()) for k in range(launches))


# ------------------------------------------------------------------ the graph searches
@functools.lru_cache(maxsize=None)
def bfs_path(n):
    """The directed path 0 -> 1 -> ... -> n - 1 as (n, rp, ci, va, x0): n steps, depth n - 1 from vertex 0."""
    rp = np.concatenate([[0], np.arange(n)]).astype(np.int32)
    ci = np.arange(n - 1, dtype=np.int32)
    x0 = np.zeros(n, np.int32)
    x0[0] = 1
    return (n,) + frozen(rp, ci, np.ones(n - 1, np.int32), x0)


@functools.lru_cache(maxsize=None)
def bfs_ref(n, cap=None):
    return BL.oracle_bfs(*bfs_path(n), max_levels=cap)


@functools.lru_cache(maxsize=None)
def core_path(R):
    """The undirected path of 2 R vertices: R peel rounds."""
    n, rp, ci, va = W.path(2 * R)
    return (n,) + frozen(rp, ci, np.ascontiguousarray(va))


@functools.lru_cache(maxsize=None)
def core_peel(R, max_rounds=None):
    return core_ref.peel(*core_path(R), max_rounds=max_rounds)


@functools.lru_cache(maxsize=None)
def truss_cliques(R):
    """Disjoint K_3 ... K_(R + 2): R peel rounds, one level and one clique per round."""
    a, b, base = [], [], 0
    for k in range(3, R + 3):
        x, y = np.triu_indices(k, 1)
        a.append(base + x)
        b.append(base + y)
        base += k
    n, rp, ci, va = T.from_pairs(base, np.concatenate(a), np.concatenate(b))
    return (n,) + frozen(rp, ci, np.ascontiguousarray(va))


@functools.lru_cache(maxsize=None)
def truss_peel(R, max_rounds=None):
    return truss_ref.peel(*truss_cliques(R), max_rounds=max_rounds)


def round_caps(R):
    return [c for c in (R - 1, R, R + 1) if c >= 1]


# ------------------------------------------------------------------ the invariant tier
SSSP_N = 128


@functools.lru_cache(maxsize=None)
def sssp_path(n=SSSP_N):
    """The directed path with unit weights and its start (0 at vertex 0) -> (n, rp, ci, va, x0)."""
    rp = np.concatenate([[0], np.arange(n)]).astype(np.int32)
    x0 = np.full(n, O.FLT_MAX, np.float32)
    x0[0] = 0.0
    return (n,) + frozen(rp, np.arange(n - 1, dtype=np.int32), np.ones(n - 1, np.float32), x0)


@functools.lru_cache(maxsize=None)
def sssp_want():
    n, rp, ci, va, x0 = sssp_path()
    dist, pred, reached, _ = sssp_ref.sssp(rp, ci, va, x0)
    return frozen(dist, pred) + (reached,)


@functools.lru_cache(maxsize=None)
def scc_path(n=40):
    """scc_ref.path(n): without trim and pivot, n colouring rounds, one vertex and a propagation sweep per hop each."""
    n, rp, ci, va = scc_ref.path(n)
    return (n,) + frozen(rp, ci, np.ascontiguousarray(va))


@functools.lru_cache(maxsize=None)
def scc_want():
    return frozen(scc_ref.components(*scc_path()))[0]


WCC_SAMPLES = (6, 7, 8, 22, 23, 24, 25)
WCC_SIDE = 32


@functools.lru_cache(maxsize=None)
def wcc_grid():
    n, rp, ci, va = W.grid(WCC_SIDE)
    return (n,) + frozen(rp, ci, np.ascontiguousarray(va))


@functools.lru_cache(maxsize=None)
def wcc_want():
    return frozen(W.components(*wcc_grid()))[0]
