"""ctypes face of libsparseharness_host.so (no HIP): the product's MatrixMarket
loader (host/src/sparse_matrix.cpp), the seeded synthetic generators
(host/src/synth.cpp) that define the benchmark configs of BASELINE.json, and the
host golds of sh_scc (host/src/scc_labels.cpp), sh_wcc (host/src/wcc_labels.cpp), sh_tri
(host/src/triangle_counts.cpp), sh_core (host/src/core_numbers.cpp), sh_truss (host/src/truss_numbers.cpp), sh_color
(host/src/greedy_colors.cpp), sh_msf (host/src/msf_edges.cpp), sh_match (host/src/greedy_matching.cpp), sh_rcm (host/src/rcm_order.cpp), sh_bc (host/src/bc_scores.cpp), sh_trsv (host/src/trsv_solve.cpp) and sh_ilu0 (host/src/ilu0_factor.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparseharness_host.so")
HOST_DIR = os.path.join(_HERE, "host")

# seeds and shapes fixed by SURVEY.md 8d / BASELINE.md
SEED_RMAT = 0x5EED0023
SEED_POWERLAW = 0x5EED1000
SEED_SCIRCUIT = 0x5EED5C1C


class _HostCsr(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("header_nnz", C.c_int32), ("nnz", C.c_int64),
                ("row_ptr", C.POINTER(C.c_int32)), ("col_idx", C.POINTER(C.c_int32)), ("val", C.c_void_p)]


_vp, _i64 = C.c_void_p, C.c_int64
_csr = [_i64, _i64, _vp, _vp, _vp]   # rows, nnz, row_ptr, col_idx, val: what every host gold starts with
# name -> (restype, argtypes): what load() binds (declared in host/inc/sh_host.h)
SIGNATURES = {
    "sh_synth_powerlaw": (C.c_int, [_i64, _i64, _i64, C.c_double, _i64, C.c_uint64, _vp, _vp, _vp]),
    "sh_synth_rmat": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint64, C.c_int, _vp, _vp, _vp]),
    "sh_scc_labels": (C.c_int, _csr + [_vp]),
    "sh_wcc_labels": (C.c_int, _csr + [_vp]),
    "sh_triangle_counts": (C.c_int, _csr + [_vp, _vp]),
    "sh_core_numbers": (C.c_int, _csr + [_vp, _vp, C.POINTER(_i64)]),
    "sh_truss_numbers": (C.c_int, _csr + [_vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "sh_greedy_colors": (C.c_int, _csr + [C.c_int32, C.c_uint32, _vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(_i64)]),
    "sh_msf_edges": (C.c_int, _csr + [_vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sh_greedy_matching": (C.c_int, _csr + [C.c_int32, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "sh_rcm_order": (C.c_int, _csr + [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(_i64), _i64, _vp, _vp, _vp, C.POINTER(_i64)]),
    "sh_bc_scores": (C.c_int, _csr + [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sh_trsv_solve": (C.c_int, _csr + [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "sh_trsv_list_sum": (C.c_double, [_vp, _i64, C.c_int32]),
    "sh_ilu0_factor": (C.c_int, _csr + [C.c_int32, _vp, _vp, _vp]),
    "sh_mm_load": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(_HostCsr)]),
    "sh_mm_load_ex": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(_HostCsr)]),
    "sh_host_csr_release": (None, [C.POINTER(_HostCsr)]),
}

_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", HOST_DIR, "../libsparseharness_host.so"])


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {HOST_DIR}`")
        os.environ.setdefault("SH_QUIET_TIMERS", "1")
        _lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = res, args
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def powerlaw(rows, nnz, cols=None, exponent=2.1, dmax=1_000_000, seed=SEED_POWERLAW):
    """Power-law row degrees, uniform columns, integer weights in [1,16] (config 5)."""
    cols = rows if cols is None else cols
    rp = np.empty(rows + 1, np.int32)
    ci = np.empty(nnz, np.int32)
    va = np.empty(nnz, np.float32)
    rc = load().sh_synth_powerlaw(rows, cols, nnz, exponent, min(dmax, cols), seed, _p(rp), _p(ci), _p(va))
    if rc:
        raise RuntimeError(f"sh_synth_powerlaw failed: {rc}")
    return rp, ci, va


def rmat(scale, edge_factor=16, a=0.57, b=0.19, c=0.19, seed=SEED_RMAT, permute=True):
    """Graph500 R-MAT (configs 3/4): 2^scale rows, edge_factor*2^scale entries, duplicates kept."""
    n = 1 << scale
    m = n * edge_factor
    rp = np.empty(n + 1, np.int32)
    ci = np.empty(m, np.int32)
    va = np.empty(m, np.float32)
    rc = load().sh_synth_rmat(scale, edge_factor, a, b, c, seed, int(permute), _p(rp), _p(ci), _p(va))
    if rc:
        raise RuntimeError(f"sh_synth_rmat failed: {rc}")
    return rp, ci, va


def scircuit_like(seed=SEED_SCIRCUIT):
    """Stand-in of SuiteSparse scircuit's shape (config 2): 170 998 rows, 958 936 entries, max row 353."""
    return powerlaw(170_998, 958_936, dmax=353, seed=seed)


def _gold(name, row_ptr, col_idx, val, *outs):
    """Run the host gold `name` over the CSR arrays of a square matrix; outs: the pointers it writes its results through."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    val = np.ascontiguousarray(val)
    assert val.dtype.itemsize == 4 and len(val) == len(col_idx)
    rc = getattr(load(), name)(len(row_ptr) - 1, len(col_idx), _p(row_ptr), _p(col_idx), _p(val), *outs)
    if rc:
        raise RuntimeError(f"{name} failed: {rc}")


def scc_labels(row_ptr, col_idx, val):
    """label[v] = the largest vertex index of v's strongly connected component (Engine.scc's comp), by a single-threaded
    Tarjan on the host.  Entry (r, c) is the edge c -> r when 0 <= c < rows and its 32 value bits are not all zero."""
    label = np.empty(len(row_ptr) - 1, np.int32)
    _gold("sh_scc_labels", row_ptr, col_idx, val, _p(label))
    return label


def wcc_labels(row_ptr, col_idx, val):
    """label[v] = the largest vertex index of v's weakly connected component (Engine.wcc's comp), by a single-threaded
    union-find on the host.  Entry (r, c) joins r and c when 0 <= c < rows and its 32 value bits are not all zero."""
    label = np.empty(len(row_ptr) - 1, np.int32)
    _gold("sh_wcc_labels", row_ptr, col_idx, val, _p(label))
    return label


def triangle_counts(row_ptr, col_idx, val):
    """-> (tri, deg): tri[v] (uint64) = the triangles through v of the simple undirected graph under the entries,
    deg[v] (int32) = its degree there (Engine.triangles' tri and deg), by a single-threaded forward algorithm on the
    host.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not all zero."""
    n = len(row_ptr) - 1
    tri, deg = np.empty(n, np.uint64), np.empty(n, np.int32)
    _gold("sh_triangle_counts", row_ptr, col_idx, val, _p(tri), _p(deg))
    return tri, deg


def core_numbers(row_ptr, col_idx, val):
    """-> (core, deg, M): core[v] (int32) = the core number of v in the simple undirected graph under the entries,
    deg[v] (int32) = its degree there (Engine.core_numbers' core and deg), M = the number of edges, by the single-threaded
    bucket algorithm of Batagelj and Zaversnik on the host.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32
    value bits are not all zero."""
    n = len(row_ptr) - 1
    core, deg, m = np.empty(n, np.int32), np.empty(n, np.int32), C.c_int64()
    _gold("sh_core_numbers", row_ptr, col_idx, val, _p(core), _p(deg), C.byref(m))
    return core, deg, m.value


def truss_numbers(row_ptr, col_idx, val):
    """-> (edge_u, edge_v, support, truss, M): for edge e of the simple undirected graph under the entries -- the e-th
    smallest pair (u, v) with u < v -- its ends, the triangles through it and its truss number (Engine.truss_numbers'
    edge_u, edge_v, support and truss; all int32), M = the number of edges, by the single-threaded bucket algorithm of
    Wang and Cheng on the host.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not all zero."""
    cap = max(len(col_idx), 1)   # (M <= nnz)
    eu, ev, sup, truss = (np.empty(cap, np.int32) for _ in range(4))
    m = C.c_int64()
    _gold("sh_truss_numbers", row_ptr, col_idx, val, _p(eu), _p(ev), _p(sup), _p(truss), C.byref(m))
    return eu[:m.value].copy(), ev[:m.value].copy(), sup[:m.value].copy(), truss[:m.value].copy(), m.value


def greedy_colors(row_ptr, col_idx, val, order=0, seed=0, prio=None):
    """-> (color, colors, depth): color[v] (int32) = the smallest colour >= 0 that no neighbour preceding v holds in the
    simple undirected graph under the entries (Engine.greedy_colors' color), colors = the largest colour plus 1,
    depth[v] (int32) = the round in which Engine.greedy_colors colours v (the longest chain of preceding neighbours that
    ends in v, counted from 0), by one serial first-fit loop on the host.  The order is sh_color's: order 0 natural, 1
    random by mix32(v ^ seed), 2 largest degree first; prio (int32 per vertex) replaces the primary key.  Entry (r, c)
    counts when 0 <= c < rows, c != r and its 32 value bits are not all zero."""
    n = len(row_ptr) - 1
    color, depth, colors = np.empty(n, np.int32), np.empty(n, np.int32), C.c_int32()
    if prio is not None:
        prio = np.ascontiguousarray(prio, np.int32)
        assert len(prio) >= n
    _gold("sh_greedy_colors", row_ptr, col_idx, val, int(order), int(seed) & 0xFFFFFFFF, None if prio is None else _p(prio),
          _p(color), _p(depth), C.byref(colors), None)
    return color, colors.value, depth


def msf_edges(row_ptr, col_idx, val):
    """-> (edge_u, edge_v, weight, in_msf, comp, M, components): for edge e of the simple undirected graph under the
    entries -- the e-th smallest pair (u, v) with u < v -- its ends (int32), the 32 bits of its weight (uint32: the
    smallest entry of the edge under the total order of the bit patterns) and whether it is in the minimum spanning
    forest under KEY(e) = k(weight[e]) << 32 | e (int32, 1 or 0); comp[v] (int32) = the largest vertex index of v's
    component (Engine.spanning_forest's outputs), M = the number of edges, by a single-threaded Kruskal with a union-find
    on the host.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not all zero."""
    n = len(row_ptr) - 1
    cap = max(len(col_idx), 1)   # (M <= nnz)
    eu, ev, msf = (np.empty(cap, np.int32) for _ in range(3))
    w, comp = np.empty(cap, np.uint32), np.empty(max(n, 1), np.int32)
    m, k = C.c_int64(), C.c_int64()
    _gold("sh_msf_edges", row_ptr, col_idx, val, _p(eu), _p(ev), _p(w), _p(msf), _p(comp), C.byref(m), C.byref(k))
    return eu[:m.value].copy(), ev[:m.value].copy(), w[:m.value].copy(), msf[:m.value].copy(), comp[:n].copy(), m.value, k.value


def greedy_matching(row_ptr, col_idx, val, heavy=1, seed=1):
    """-> (edge_u, edge_v, weight, in_match, mate, M, pairs): the edges of the simple undirected graph under the entries
    as msf_edges gives them, whether edge e is matched (int32, 1 or 0) and mate[v] (int32) = the partner of v or -1
    (Engine.matching's outputs), by a single-threaded loop on the host that takes the edges in ascending MKEY and keeps
    an edge when both its ends are still free.  MKEY(e) = hi << 32 | lo with hi = k(weight[e]) for heavy == 0 and its
    complement for heavy == 1, lo = e for seed == 0 and mix32(e ^ seed) otherwise."""
    n = len(row_ptr) - 1
    cap = max(len(col_idx), 1)   # (M <= nnz)
    eu, ev, chosen = (np.empty(cap, np.int32) for _ in range(3))
    w, mate = np.empty(cap, np.uint32), np.empty(max(n, 1), np.int32)
    m, k = C.c_int64(), C.c_int64()
    _gold("sh_greedy_matching", row_ptr, col_idx, val, int(heavy), int(seed) & 0xFFFFFFFF, _p(eu), _p(ev), _p(w), _p(chosen),
          _p(mate), C.byref(m), C.byref(k))
    return eu[:m.value].copy(), ev[:m.value].copy(), w[:m.value].copy(), chosen[:m.value].copy(), mate[:n].copy(), m.value, k.value


def rcm_order(row_ptr, col_idx, val, sweeps=8, reverse=1, records=False):
    """-> (perm, pos, level, bandwidth_before, bandwidth_after, profile_before, profile_after, components, searches), and
    with records (kinds, sizes, edges) behind them -- per step, i.e. per level of every search from a vertex with an
    edge: 0 for a root search and 1 for the numbering, the level's width, the sum of its list lengths --:
    perm[k] (int32) = the vertex at new position k under the reverse Cuthill-McKee ordering of the simple undirected
    graph under the entries (Engine.rcm_order's perm; A[perm][:, perm] is the reordered matrix), pos its inverse,
    level[v] the level of v from its component's root, bandwidth and profile under the identity and under the new order,
    the components and the searches run to find roots, by the serial definition on the host: the vertices walked in
    ascending (deg, index), each component's root by George and Liu's searches (at most `sweeps` beyond the first; 0: the
    first vertex of the walk), the numbering with one queue and every list in ascending (deg, index).  Entry (r, c)
    counts when 0 <= c < rows, c != r and its 32 value bits are not all zero."""
    n = len(row_ptr) - 1
    perm, pos, level = (np.empty(max(n, 1), np.int32) for _ in range(3))
    bw, prof = np.zeros(2, np.int64), np.zeros(2, np.int64)
    comps, searches = C.c_int32(), C.c_int32()
    cap = (int(sweeps) + 2) * n + 1 if records else 0   # (a run has at most (sweeps + 2) * rows steps)
    kinds, sizes, edges, steps = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int64), _i64()
    _gold("sh_rcm_order", row_ptr, col_idx, val, int(sweeps), int(reverse), _p(perm), _p(pos), _p(level), _p(bw), _p(prof),
          C.byref(comps), C.byref(searches), None, cap, _p(kinds), _p(sizes), _p(edges), C.byref(steps))
    out = (perm[:n].copy(), pos[:n].copy(), level[:n].copy(), int(bw[0]), int(bw[1]), int(prof[0]), int(prof[1]), comps.value,
           searches.value)
    k = steps.value
    return out + (kinds[:k].copy(), sizes[:k].copy(), edges[:k].copy()) if records else out


def bc_scores(row_ptr, col_idx, val, sources, bc=None):
    """-> (bc, sigma, level, depths, reached, sigma_max, edges): bc[v] (float64) = the betweenness of v in the simple
    directed graph under the entries, summed over `sources` in the order given (Engine.betweenness's bc; `bc`: scores to
    add to, as accumulate = 1), sigma (float64) and level (int32) of the last source, and per source the last level that
    holds a vertex, the vertices reached, the largest path count and the out-list entries walked forward, by a serial
    Brandes on the host whose every float64 sum runs in the order include/sparseharness_hip.h fixes: the results are
    sh_bc's bit for bit.  Entry (r, c) is the edge c -> r when 0 <= c < rows, c != r and its 32 value bits are not all
    zero."""
    n = len(row_ptr) - 1
    sources = np.ascontiguousarray(sources, np.int32)
    k = len(sources)
    out = np.zeros(max(n, 1), np.float64) if bc is None else np.array(bc, np.float64)
    assert len(out) >= n
    sigma, level = np.zeros(max(n, 1), np.float64), np.full(max(n, 1), -1, np.int32)
    depths, reached = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int64)
    smax, edges = np.zeros(max(k, 1), np.float64), np.zeros(max(k, 1), np.int64)
    _gold("sh_bc_scores", row_ptr, col_idx, val, _p(sources), k, 0 if bc is None else 1, _p(out), _p(sigma), _p(level),
          _p(depths), _p(reached), _p(smax), _p(edges))
    return out[:n], sigma[:n], level[:n], depths[:k], reached[:k], smax[:k], edges[:k]


def trsv_solve(row_ptr, col_idx, val, b, uplo=0, unit=0, f32=0):
    """-> (x, level, figures): x (float64, or float32 when f32) = the solution of T x = b for the triangle `uplo` (0 lower,
    1 upper) of the square matrix, its diagonal taken as one when `unit` (Engine.trsv's x), level[r] (int32) = 0 for an
    empty list, else 1 + the largest level in r's list, and figures = dict(entries, levels, max_list, max_width,
    zero_diag, first_zero) (the getters of trsv.TrsvGraph), by plain substitution on the host whose every float64 sum
    runs in the order include/sparseharness_hip.h fixes: the results are sh_trsv's bit for bit.  Every stored entry with
    0 <= c < rows takes part whatever its value; parallel entries are separate terms."""
    n = len(row_ptr) - 1
    b = np.ascontiguousarray(b, np.float32 if f32 else np.float64)
    assert len(b) >= n
    x = np.zeros(max(n, 1), b.dtype)
    level, fig = np.zeros(max(n, 1), np.int32), np.zeros(6, np.int64)
    _gold("sh_trsv_solve", row_ptr, col_idx, val, _p(b), int(uplo), int(unit), int(f32), _p(x), _p(level), _p(fig))
    names = ("entries", "levels", "max_list", "max_width", "zero_diag", "first_zero")
    return x[:n], level[:n], dict(zip(names, (int(v) for v in fig)))


def trsv_list_sum(terms, tier=0):
    """SUM of signed float64 terms as sh_trsv defines it (tier 0: as sh_trsv chooses; 1: the one-lane formula, at most 8
    terms; 2: the pieces)."""
    t = np.ascontiguousarray(terms, np.float64)
    return float(load().sh_trsv_list_sum(_p(t), len(t), int(tier)))


def ilu0_factor(row_ptr, col_idx, val, f32=1):
    """-> (lu, level, figures): lu (float32 when f32, else float64) = the ILU(0) factor of the square matrix in the
    positions of its entries (Engine.ilu0's lu: the slot's value at the first entry of its (r, c) group, +0.0 at a later
    one or at a column outside the matrix), level[r] (int32) = 0 for a row without a lower slot, else 1 + the largest level
    among its lower slots, and figures = dict(entries, levels, max_list, max_width, missing_diag, first_missing, work,
    zero_pivots, first_zero) (the getters of ilu0.Ilu0Graph and the figures of a call), by the row-wise IKJ recurrence on
    the host in the order include/sparseharness_hip.h fixes: the results are sh_ilu0's bit for bit."""
    n = len(row_ptr) - 1
    lu = np.zeros(max(len(col_idx), 1), np.float32 if f32 else np.float64)
    level, fig = np.zeros(max(n, 1), np.int32), np.zeros(9, np.int64)
    _gold("sh_ilu0_factor", row_ptr, col_idx, val, int(f32), _p(lu), _p(level), _p(fig))
    names = ("entries", "levels", "max_list", "max_width", "missing_diag", "first_missing", "work", "zero_pivots", "first_zero")
    return lu[:len(col_idx)], level[:n], dict(zip(names, (int(v) for v in fig)))


NORM_NONE, NORM_PAGERANK, NORM_SCC = 0, 1, 2


def mm_load(path, elem_is_int=False, truncate=True, normalise=NORM_NONE, damping=0.85):
    """MatrixMarket -> (rows, cols, header_nnz, row_ptr, col_idx, val) through the product loader;
    normalise applies SparseMatrix::pagerank_normalise / scc_normalise as the pr / scc apps do."""
    m = _HostCsr()
    rc = load().sh_mm_load_ex(os.fsencode(path), int(elem_is_int), int(truncate), int(normalise), float(damping),
                              C.byref(m))
    if rc:
        raise RuntimeError(f"sh_mm_load({path}) failed: {rc}")
    try:
        rp = np.ctypeslib.as_array(m.row_ptr, (m.rows + 1,)).copy()
        ci = np.ctypeslib.as_array(m.col_idx, (max(m.nnz, 1),))[:m.nnz].copy()
        vt = C.c_int32 if elem_is_int else C.c_float
        va = np.ctypeslib.as_array(C.cast(m.val, C.POINTER(vt)), (max(m.nnz, 1),))[:m.nnz].copy()
    finally:
        load().sh_host_csr_release(C.byref(m))
    return m.rows, m.cols, m.header_nnz, rp, ci, va
