"""Thin Python face of the C ABI (include/sparseharness_hip.h) for tests and bench.

Everything here forwards to the HIP engine through ctypes; there is no Python
or CPU compute path.  Names follow the reference's domain: matrix, x/y/output
vectors, semiring, run (launch geometry), trials.
"""
import ctypes as C

import numpy as np

from . import abi
from .abi import MAX_MIN_I32, MIN_PLUS_F32, OR_AND_I32, PLUS_TIMES_F32  # noqa: F401

FLT_MAX = np.float32(3.4028235e38)


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[sh error {code}] {msg}")
        self.code = code


def elem_dtype(semiring):
    return np.int32 if semiring in (OR_AND_I32, MAX_MIN_I32) else np.float32


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _csr_args(row_ptr, col_idx, val):
    """The CSR arrays as the engine reads them: contiguous, int32 indices, values of 4 bytes."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    val = np.ascontiguousarray(val)
    assert val.dtype.itemsize == 4
    return row_ptr, col_idx, val


_CTYPE_OF = {np.int32: C.c_int32, np.int64: C.c_int64, np.uint64: C.c_uint64, np.float64: C.c_double}


def _outs(cap, *dtypes):
    """(arrays, pointers): one zeroed host array of `cap` elements per dtype for the per-round figures of a driver, and
    the typed pointers the engine writes them through."""
    arrays = tuple(np.zeros(cap, dt) for dt in dtypes)
    return arrays, tuple(a.ctypes.data_as(C.POINTER(_CTYPE_OF[dt])) for a, dt in zip(arrays, dtypes))


class Vec:
    """Device vector of 4-byte elements (x, y, output of the harness)."""

    def __init__(self, engine, handle, owned=True):
        self.engine, self.h, self.owned = engine, handle, owned

    def __len__(self):
        return abi.load().sh_vec_len(self.h)

    @property
    def device_ptr(self):
        return abi.load().sh_vec_device_ptr(self.h)

    def upload(self, host):
        host = np.ascontiguousarray(host)
        assert host.dtype.itemsize == 4
        self.engine._chk(abi.load().sh_vec_upload(self.engine.h, self.h, _ptr(host), host.size))
        return self

    def download(self, dtype=np.float32, n=None, shape=None):
        """shape=(rows, width): the interleaved vectors of Engine.spmm as a C-contiguous 2-D array."""
        if shape is not None:
            n = int(np.prod(shape))
        n = len(self) if n is None else n
        out = np.empty(n, dtype)
        self.engine._chk(abi.load().sh_vec_download(self.engine.h, self.h, _ptr(out), n))
        return out if shape is None else out.reshape(shape)

    def fill(self, value, dtype=np.float32):
        pat = int(np.array([value], dtype).view(np.uint32)[0])
        self.engine._chk(abi.load().sh_vec_fill(self.engine.h, self.h, pat))
        return self

    def free(self):
        if self.h is not None:
            abi.load().sh_vec_free(self.engine.h, self.h)
            self.h = None


class CsrMatrix:
    """Device-resident CSR matrix + launch schedule (replaces cl_encode's buffers)."""

    def __init__(self, engine, handle, rows, cols, nnz):
        self.engine, self.h = engine, handle
        self.rows, self.cols, self.nnz = rows, cols, nnz

    def algorithmic_bytes(self, reads_y=False):
        b = C.c_uint64()
        self.engine._chk(abi.load().sh_csr_algorithmic_bytes(self.h, int(reads_y), C.byref(b)))
        return b.value

    def plan(self):
        """('stream'|'tiled'|'bits', HBM bytes one SpMV streams by construction)."""
        p, b = C.c_int32(), C.c_uint64()
        self.engine._chk(abi.load().sh_csr_plan(self.h, C.byref(p), C.byref(b)))
        return ("stream", "tiled", "bits")[p.value], b.value

    def describe(self):
        """One-line description of the device layout (plan, value coding, tile/bin counts)."""
        buf = C.create_string_buffer(256)
        self.engine._chk(abi.load().sh_csr_describe(self.h, buf, len(buf)))
        return buf.value.decode()

    def footprint(self):
        """Device bytes held by this matrix."""
        b = C.c_uint64()
        self.engine._chk(abi.load().sh_csr_footprint(self.h, C.byref(b)))
        return b.value

    def builder(self):
        """("host" | "device", note): who built the tiled layout, and why the device builder was not used if asked for."""
        w, note = C.c_int32(), C.create_string_buffer(256)
        self.engine._chk(abi.load().sh_csr_builder(self.h, C.byref(w), note, len(note)))
        return ("device" if w.value else "host"), note.value.decode()

    def placement(self):
        """(placements of the big arrays timed at upload, ms of the first, ms of the one kept)."""
        n, a, b = C.c_int32(), C.c_float(), C.c_float()
        self.engine._chk(abi.load().sh_csr_placement(self.h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, round(a.value, 4), round(b.value, 4)

    def free(self):
        if self.h is not None:
            abi.load().sh_csr_free(self.engine.h, self.h)
            self.h = None


class _Handle:
    """A device-side handle made by the engine: `h` is the C handle, `n` its rows, `_c` the prefix of its C functions
    (<_c>_create, <_c>_free, <_c>_footprint, ...)."""
    _c = None

    def __init__(self, engine, handle, n):
        self.engine, self.h, self.n = engine, handle, n

    def _get(self, suffix, ctype):
        """What <_c>_<suffix> writes through its one out-pointer."""
        v = ctype()
        self.engine._chk(getattr(abi.load(), f"{self._c}_{suffix}")(self.h, C.byref(v)))
        return v.value

    def free(self):
        if self.h is not None:
            getattr(abi.load(), self._c + "_free")(self.engine.h, self.h)
            self.h = None


def _getter(suffix, ctype, doc):
    """The read-only property behind <_c>_<suffix> (tests/test_abi.py checks `reads` against abi.SIGNATURES)."""
    def get(self):
        return self._get(suffix, ctype)
    get.reads = (suffix, ctype)
    return property(get, doc=doc)


class _Graph(_Handle):
    """A handle made from the host CSR arrays alone (Engine._graph): it needs no CsrMatrix."""
    edges = _getter("edges", C.c_int64, "Entries kept as edges (non-zero value bits, column inside the matrix).")
    footprint = _getter("footprint", C.c_uint64, "Device bytes held by the handle (the formula: include/sparseharness_hip.h).")


class Frontier(_Handle):
    """What the sparse launches of Engine.iterate_frontier need for one square matrix: its CSR arrays (borrowed from
    the matrix when it keeps them, copied otherwise), the pattern of its transpose, worklists."""
    _c = "sh_frontier"

    def transpose(self):
        """(col_ptr[n + 1], row_of[col_ptr[n]]); the order of the rows inside one column is unspecified."""
        lib = abi.load()
        col_ptr = np.zeros(self.n + 1, np.int32)
        self.engine._chk(lib.sh_frontier_transpose(self.engine.h, self.h, col_ptr.ctypes.data_as(C.POINTER(C.c_int32)), None))
        row_of = np.zeros(max(int(col_ptr[-1]), 1), np.int32)
        self.engine._chk(lib.sh_frontier_transpose(self.engine.h, self.h, None, row_of.ctypes.data_as(C.POINTER(C.c_int32))))
        return col_ptr, row_of[:int(col_ptr[-1])]

    def footprint(self):
        """Device bytes held by the handle (the formula: include/sparseharness_hip.h)."""
        return self._get("footprint", C.c_uint64)


class BfsGraph(_Graph):
    """What Engine.bfs_levels searches: the edge pattern of a square matrix by rows and its transpose, queues, bitmaps
    (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_bfs_graph"


class SsspGraph(_Graph):
    """What Engine.sssp searches: the weighted out-edges of a square matrix by source vertex, its in-edges by row, work
    lists (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_sssp_graph"
    edges = _getter("edges", C.c_int64,
                    "Entries kept as edges (finite value, column inside the matrix; a stored zero is an edge of weight 0).")
    delta = _getter("delta", C.c_double, "The default bucket width (0 for a graph without edges).")


class SccGraph(_Graph):
    """What Engine.scc searches: the edge pattern of a square matrix by rows and its transpose, colours, work lists
    (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_scc_graph"


class WccGraph(_Graph):
    """What Engine.wcc searches: the edge pattern of a square matrix by rows and its transpose, a parent word per vertex,
    a work list (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_wcc_graph"


class TriGraph(_Graph):
    """What Engine.triangles counts in: the simple undirected graph under the entries of a square matrix, oriented, as
    ascending forward lists, with its degrees (made from the host CSR arrays alone; needs no CsrMatrix)."""
    _c = "sh_tri_graph"
    edges = _getter("edges", C.c_int64, "M: the edges of the simple undirected graph.")
    max_forward = _getter("max_forward", C.c_int64, "The length of the longest forward list.")


class CoreGraph(_Graph):
    """What Engine.core_numbers peels: the simple undirected graph under the entries of a square matrix as symmetric
    ascending lists, with its degrees, the remaining degrees of a call and two work lists (made from the host CSR
    arrays alone; needs no CsrMatrix)."""
    _c = "sh_core_graph"
    edges = _getter("edges", C.c_int64, "M: the edges of the simple undirected graph.")
    max_degree = _getter("max_degree", C.c_int64, "The largest degree (the length of the longest list).")


class Engine:
    """One HIP device + one stream (replaces Harness's OpenCL context/queue)."""

    def __init__(self, device=0, stream=None):
        lib = abi.load()
        h = C.c_void_p()
        if stream is None:
            rc = lib.sh_engine_create(device, C.byref(h))
        else:
            rc = lib.sh_engine_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if rc != abi.SH_OK:
            raise EngineError(rc, (lib.sh_last_error(None) or b"").decode())
        self.h = h
        self.device = device

    def _chk(self, rc):
        if rc != abi.SH_OK:
            raise EngineError(rc, (abi.load().sh_last_error(self.h) or b"").decode())

    def close(self):
        if self.h is not None:
            abi.load().sh_engine_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        self._chk(abi.load().sh_engine_device_name(self.h, buf, 256))
        return buf.value.decode()

    def max_alloc(self):
        b = C.c_uint64()
        self._chk(abi.load().sh_engine_max_alloc(self.h, C.byref(b)))
        return b.value

    def synchronize(self):
        self._chk(abi.load().sh_engine_synchronize(self.h))

    # ---- buffers
    def upload_csr(self, rows, cols, row_ptr, col_idx, val, **options):
        """options: fields of sh_plan_options (plan=0|1|2, value_coding=0|8|-1, fold=0, ...) on top of the
        SH_* environment; without any the environment alone decides (sh_csr_upload)."""
        row_ptr, col_idx, val = _csr_args(row_ptr, col_idx, val)
        nnz = int(row_ptr[-1]) if len(row_ptr) else 0
        h = C.c_void_p()
        lib = abi.load()
        if options:
            opt = abi.sh_plan_options()
            lib.sh_plan_options_from_env(C.byref(opt))
            for k, v in options.items():
                setattr(opt, k, v)
            self._chk(lib.sh_csr_upload_ex(self.h, rows, cols, nnz, _ptr(row_ptr), _ptr(col_idx), _ptr(val),
                                           C.byref(opt), C.byref(h)))
        else:
            self._chk(lib.sh_csr_upload(self.h, rows, cols, nnz, _ptr(row_ptr), _ptr(col_idx), _ptr(val), C.byref(h)))
        return CsrMatrix(self, h, rows, cols, nnz)

    def alloc(self, n):
        h = C.c_void_p()
        self._chk(abi.load().sh_vec_alloc(self.h, n, C.byref(h)))
        return Vec(self, h)

    def wrap(self, device_ptr, n):
        h = C.c_void_p()
        self._chk(abi.load().sh_vec_wrap(self.h, C.c_void_p(device_ptr), n, C.byref(h)))
        return Vec(self, h, owned=False)

    def vector(self, host):
        host = np.ascontiguousarray(host)
        return self.alloc(host.size).upload(host)

    # ---- hot path
    def spmv(self, semiring, A, x, y, alpha, beta, out, timed=False, run=None):
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        ns = C.c_uint64()
        launch = None
        if run is not None:
            launch = abi.sh_launch()
            launch.global_[:] = run[:3]
            launch.local[:] = run[3:]
        self._chk(abi.load().sh_spmv(self.h, semiring, A.h, x.h, None if y is None else y.h, _ptr(a),
                                     _ptr(b), out.h, launch, C.byref(ns) if timed else None))
        return ns.value if timed else None

    def step(self, semiring, A, x, y, alpha, beta, out, x_row_offset=0, delta=1e-4, changed_ptr=None):
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        self._chk(abi.load().sh_spmv_step(self.h, semiring, A.h, x.h, None if y is None else y.h, _ptr(a),
                                          _ptr(b), out.h, x_row_offset, delta,
                                          None if changed_ptr is None else C.c_void_p(changed_ptr)))

    def iterate(self, semiring, A, x, y0, scratch, alpha, beta, delta=1e-4, max_iters=10000):
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        iters, conv, total = C.c_int32(), C.c_int32(), C.c_uint64()
        per = (C.c_uint64 * max_iters)()
        self._chk(abi.load().sh_iterate(self.h, semiring, A.h, x.h, y0.h, scratch.h, _ptr(a), _ptr(b),
                                        delta, max_iters, None, C.byref(iters), C.byref(conv), per,
                                        C.byref(total)))
        return iters.value, bool(conv.value), list(per[:iters.value]), total.value

    # ---- frontier-driven iteration: only the rows whose inputs changed are recomputed while the wavefront is thin
    def frontier(self, A, row_ptr, col_idx, val):
        """The handle Engine.iterate_frontier needs; the arrays are the ones A was uploaded from (A must outlive it)."""
        row_ptr, col_idx, val = _csr_args(row_ptr, col_idx, val)
        h = C.c_void_p()
        self._chk(abi.load().sh_frontier_create(self.h, A.h, int(row_ptr[-1]), _ptr(row_ptr), _ptr(col_idx), _ptr(val), C.byref(h)))
        return Frontier(self, h, A.rows)

    def iterate_frontier(self, semiring, A, F, x, y0, scratch, alpha, beta, delta=1e-4, max_iters=10000, dense_share=-1.0):
        """-> (iters, converged, modes, changed, active, ns_per_iter, total_ns); per launch: 0 dense / 1 sparse, rows whose
        bits it changed, rows it recomputed."""
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        iters, conv, total = C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_iters), 1)
        per, modes = (C.c_uint64 * cap)(), (C.c_int32 * cap)()
        changed, active = (C.c_int64 * cap)(), (C.c_int64 * cap)()
        self._chk(abi.load().sh_iterate_frontier(self.h, semiring, A.h, F.h, x.h, y0.h, scratch.h, _ptr(a), _ptr(b), delta,
                                                 max_iters, dense_share, C.byref(iters), C.byref(conv), modes, changed, active,
                                                 per, C.byref(total)))
        n = iters.value
        return n, bool(conv.value), list(modes[:n]), list(changed[:n]), list(active[:n]), list(per[:n]), total.value

    def _graph(self, cls, row_ptr, col_idx, val, *extra):
        """A cls from the CSR arrays of a square matrix, by <cls._c>_create (extra: what it takes between val and out)."""
        row_ptr, col_idx, val = _csr_args(row_ptr, col_idx, val)
        h = C.c_void_p()
        self._chk(getattr(abi.load(), cls._c + "_create")(self.h, len(row_ptr) - 1, len(col_idx), _ptr(row_ptr), _ptr(col_idx),
                                                          _ptr(val), *extra, C.byref(h)))
        return cls(self, h, len(row_ptr) - 1)

    # ---- direction-optimising BFS: the level of every vertex and, on request, its canonical parent
    def bfs_graph(self, row_ptr, col_idx, val):
        """The handle Engine.bfs_levels needs, from the CSR arrays of a square matrix."""
        return self._graph(BfsGraph, row_ptr, col_idx, val)

    def bfs_levels(self, G, x0, level, parent=None, max_levels=1 << 20, up_share=-1.0, down_share=-1.0):
        """-> (depth, reached, complete, modes, sizes, edges, ns_per_level, total_ns); per step that ran: 0 top-down /
        1 bottom-up, edges it looked at, device ns; sizes[l] = vertices at level l (one entry more than the steps)."""
        depth, reached, complete, total = C.c_int32(), C.c_int64(), C.c_int32(), C.c_uint64()
        cap = max(int(max_levels), 1)
        (modes, edges, per), (p_modes, p_edges, p_per) = _outs(cap, np.int32, np.int64, np.uint64)
        (sizes,), (p_sizes,) = _outs(cap + 1, np.int64)
        sizes[:] = -1
        self._chk(abi.load().sh_bfs_levels(self.h, G.h, x0.h, level.h, None if parent is None else parent.h, max_levels,
                                           up_share, down_share, C.byref(depth), C.byref(reached), C.byref(complete),
                                           p_modes, p_sizes, p_edges, p_per, C.byref(total)))
        n = int(np.count_nonzero(sizes >= 0)) - 1   # steps that ran (sizes holds one entry per step, plus the sources)
        if n < 0:   # (a graph without rows: nothing ran and nothing was written)
            n, sizes[0] = 0, 0
        return (depth.value, reached.value, bool(complete.value), modes[:n].copy(), sizes[:n + 1].copy(), edges[:n].copy(),
                per[:n].copy(), total.value)

    # ---- bucketed SSSP: the distance of every vertex and, on request, its canonical predecessor
    def sssp_graph(self, row_ptr, col_idx, val):
        """The handle Engine.sssp needs, from the CSR arrays of a square matrix (val: float32 bit patterns)."""
        return self._graph(SsspGraph, row_ptr, col_idx, val)

    def sssp(self, G, x0, dist, pred=None, delta=-1.0, max_rounds=1 << 20):
        """-> (rounds, buckets, reached, complete, relaxed, sizes, edges, ns_per_round, total_ns); per round that ran:
        vertices relaxed from, edges looked at, device ns."""
        rounds, buckets, reached, complete = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        relaxed, total = C.c_int64(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (sizes, edges, per), ptrs = _outs(cap, np.int64, np.int64, np.uint64)
        self._chk(abi.load().sh_sssp(self.h, G.h, x0.h, dist.h, None if pred is None else pred.h, delta, max_rounds,
                                     C.byref(rounds), C.byref(buckets), C.byref(reached), C.byref(complete), C.byref(relaxed),
                                     *ptrs, C.byref(total)))
        n = rounds.value
        return (n, buckets.value, reached.value, bool(complete.value), relaxed.value, sizes[:n].copy(), edges[:n].copy(),
                per[:n].copy(), total.value)

    # ---- strongly connected components: comp[v] = the largest vertex index of v's component
    def scc_graph(self, row_ptr, col_idx, val):
        """The handle Engine.scc needs, from the CSR arrays of a square matrix."""
        return self._graph(SccGraph, row_ptr, col_idx, val)

    def scc(self, G, comp, trim=True, pivot=True, max_steps=1 << 20):
        """-> (components, settled, trimmed, rounds, steps, complete, kinds, sizes, steps_per, edges, ns, total_ns); per
        round: 0 trim / 1 pivot / 2 colouring, vertices it settled, its steps, edges it looked at, device ns."""
        components, settled, trimmed = C.c_int64(), C.c_int64(), C.c_int64()
        rounds, steps, complete, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_steps), 1)
        (kinds, sizes, steps_per, edges, per), ptrs = _outs(cap, np.int32, np.int64, np.int32, np.int64, np.uint64)
        self._chk(abi.load().sh_scc(self.h, G.h, comp.h, int(bool(trim)), int(bool(pivot)), max_steps, C.byref(components),
                                    C.byref(settled), C.byref(trimmed), C.byref(rounds), C.byref(steps), C.byref(complete), *ptrs,
                                    C.byref(total)))
        n = rounds.value
        return (components.value, settled.value, trimmed.value, n, steps.value, bool(complete.value), kinds[:n].copy(),
                sizes[:n].copy(), steps_per[:n].copy(), edges[:n].copy(), per[:n].copy(), total.value)

    # ---- weakly connected components: comp[v] = the largest vertex index of v's weak component
    def wcc_graph(self, row_ptr, col_idx, val):
        """The handle Engine.wcc needs, from the CSR arrays of a square matrix."""
        return self._graph(WccGraph, row_ptr, col_idx, val)

    def wcc(self, G, comp, sample=2, max_rounds=1 << 20):
        """-> (components, skipped, rounds, complete, kinds, hooks, jumps, edges, ns, total_ns); per round: 0 sampling /
        1 full, compare-and-swaps won, pointers changed, entries looked at, device ns."""
        components, skipped = C.c_int64(), C.c_int64()
        rounds, complete, total = C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (kinds, hooks, jumps, edges, per), ptrs = _outs(cap, np.int32, np.int64, np.int64, np.int64, np.uint64)
        self._chk(abi.load().sh_wcc(self.h, G.h, comp.h, sample, max_rounds, C.byref(components), C.byref(skipped),
                                    C.byref(rounds), C.byref(complete), *ptrs, C.byref(total)))
        n = rounds.value
        return (components.value, skipped.value, n, bool(complete.value), kinds[:n].copy(), hooks[:n].copy(), jumps[:n].copy(),
                edges[:n].copy(), per[:n].copy(), total.value)

    # ---- triangle counts: tri[v] = the triangles through v (uint64, two 4-byte elements per vertex), deg[v] = its degree
    def tri_graph(self, row_ptr, col_idx, val, order=1):
        """The handle Engine.triangles needs, from the CSR arrays of a square matrix.  order 0: edges run from the
        smaller index to the larger; 1: from the smaller (degree, index) to the larger."""
        return self._graph(TriGraph, row_ptr, col_idx, val, order)

    def triangles(self, G, tri=None, deg=None):
        """-> (triangles, probes, total_ns).  tri: None or a vector of >= 2 * rows 4-byte elements (rows uint64 counts);
        deg: None or an int32 vector of >= rows elements."""
        count, probes, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(abi.load().sh_tri(self.h, G.h, None if tri is None else tri.h, None if deg is None else deg.h,
                                    C.byref(count), C.byref(probes), C.byref(total)))
        return count.value, probes.value, total.value

    # ---- core numbers: core[v] = the largest k such that v lies in a subgraph of minimum degree k
    def core_graph(self, row_ptr, col_idx, val):
        """The handle Engine.core_numbers needs, from the CSR arrays of a square matrix."""
        return self._graph(CoreGraph, row_ptr, col_idx, val)

    # chase = 0: the fastest arm of tools/core_bench.py on the 2048 x 2048 grid and no slower than any on R-MAT-18
    # (DESIGN.md 6j); chasing pays for chains of degree-2 vertices only
    def core_numbers(self, G, core, deg=None, chase=0, max_rounds=None):
        """-> (degeneracy, levels, rounds, complete, ks, sizes, chased, edges, ns, total_ns); per round: the level k being
        peeled, vertices taken from the work list, vertices settled inside the launch, list entries looked at, device ns.
        core: an int32 vector of >= rows elements; deg: None or one more.  max_rounds = None: rows + 1, which cannot cut
        a run short."""
        if max_rounds is None:
            max_rounds = G.n + 1
        degeneracy, levels, rounds, complete, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (ks, sizes, chased, edges, per), ptrs = _outs(cap, np.int32, np.int64, np.int64, np.int64, np.uint64)
        self._chk(abi.load().sh_core(self.h, G.h, core.h, None if deg is None else deg.h, chase, max_rounds,
                                     C.byref(degeneracy), C.byref(levels), C.byref(rounds), C.byref(complete), *ptrs, C.byref(total)))
        n = rounds.value
        return (degeneracy.value, levels.value, n, bool(complete.value), ks[:n].copy(), sizes[:n].copy(), chased[:n].copy(),
                edges[:n].copy(), per[:n].copy(), total.value)

    # ---- truss numbers: truss[e] = the largest k such that edge e lies in a subgraph whose edges are all in >= k - 2 of
    # its triangles; edge e = the e-th smallest pair (u, v), u < v
    def truss_graph(self, row_ptr, col_idx, val):
        """The handle Engine.truss_numbers needs (truss.TrussGraph), from the CSR arrays of a square matrix."""
        from .truss import TrussGraph   # (truss.py imports this module)
        return self._graph(TrussGraph, row_ptr, col_idx, val)

    def truss_numbers(self, G, truss, support=None, edge_u=None, edge_v=None, max_rounds=None):
        """-> (max_truss, levels, rounds, complete, triangles, ks, sizes, walked, ns, total_ns); per round: the k being
        peeled, edges settled, the sum of min(deg u, deg v) over them, device ns.  truss: an int32 vector of >= M = G.edges
        elements; support, edge_u, edge_v: None or one more each.  max_rounds = None: M + 1, which cannot cut a run
        short."""
        if max_rounds is None:
            max_rounds = G.edges + 1
        max_truss, levels, rounds, complete = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        triangles, total = C.c_uint64(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (ks, sizes, walked, per), ptrs = _outs(cap, np.int32, np.int64, np.int64, np.uint64)
        h = lambda v: None if v is None else v.h   # noqa: E731
        self._chk(abi.load().sh_truss(self.h, G.h, truss.h, h(support), h(edge_u), h(edge_v), max_rounds, C.byref(max_truss),
                                      C.byref(levels), C.byref(rounds), C.byref(complete), C.byref(triangles), *ptrs,
                                      C.byref(total)))
        n = rounds.value
        return (max_truss.value, levels.value, n, bool(complete.value), triangles.value, ks[:n].copy(), sizes[:n].copy(),
                walked[:n].copy(), per[:n].copy(), total.value)

    # ---- greedy colouring: color[v] = the smallest colour that no neighbour preceding v in a fixed order holds
    def color_graph(self, row_ptr, col_idx, val):
        """The handle Engine.greedy_colors needs (color.ColorGraph), from the CSR arrays of a square matrix."""
        from .color import ColorGraph   # (color.py imports this module)
        return self._graph(ColorGraph, row_ptr, col_idx, val)

    def greedy_colors(self, G, color, prio=None, order=2, seed=0, window=0, max_rounds=None):
        """-> (colors, rounds, complete, coloured, sizes, edges, ns, total_ns); per round: the vertices coloured, the sum
        of their list lengths, device ns.  color: an int32 vector of >= rows elements; prio: None or an int32 vector of
        >= rows priorities that replace the primary key.  order: 0 natural, 1 random, 2 largest degree first; window: 0
        or the colours per LDS bitmap of a long list.  max_rounds = None: rows + 1, which cannot cut a run short."""
        if max_rounds is None:
            max_rounds = G.n + 1
        colors, rounds, complete, coloured, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (sizes, edges, per), ptrs = _outs(cap, np.int64, np.int64, np.uint64)
        self._chk(abi.load().sh_color(self.h, G.h, color.h, None if prio is None else prio.h, order, seed, window, max_rounds,
                                      C.byref(colors), C.byref(rounds), C.byref(complete), C.byref(coloured), *ptrs,
                                      C.byref(total)))
        n = rounds.value
        return (colors.value, n, bool(complete.value), coloured.value, sizes[:n].copy(), edges[:n].copy(), per[:n].copy(),
                total.value)

    # ---- minimum spanning forest: in_msf[e] = 1 for the edges of the one forest that is lightest under KEY(e)
    def msf_graph(self, row_ptr, col_idx, val):
        """The handle Engine.spanning_forest needs (msf.MsfGraph), from the CSR arrays of a square matrix whose float32
        values are the weights."""
        from .msf import MsfGraph   # (msf.py imports this module)
        return self._graph(MsfGraph, row_ptr, col_idx, val)

    def spanning_forest(self, G, in_msf, comp=None, edge_u=None, edge_v=None, weight=None, max_rounds=33):
        """-> (tree_edges, components, rounds, complete, walked, kept, hooks, jumps, ns, total_ns); per round: the length
        of the edge list at its start, the edges that still joined two trees, the roots hooked, pointers changed by the
        jumps, device ns.  in_msf: an int32 vector of >= M = G.edges elements; edge_u, edge_v, weight: None or one more
        each; comp: None or an int32 vector of >= rows elements.  max_rounds = 33 can never cut a run short (a run has
        at most floor(log2(rows)) + 1 rounds)."""
        tree_edges, components = C.c_int64(), C.c_int64()
        rounds, complete, total = C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (walked, kept, hooks, jumps, per), ptrs = _outs(cap, np.int64, np.int64, np.int64, np.int64, np.uint64)
        h = lambda v: None if v is None else v.h   # noqa: E731
        self._chk(abi.load().sh_msf(self.h, G.h, in_msf.h, h(comp), h(edge_u), h(edge_v), h(weight), max_rounds,
                                    C.byref(tree_edges), C.byref(components), C.byref(rounds), C.byref(complete), *ptrs,
                                    C.byref(total)))
        n = rounds.value
        return (tree_edges.value, components.value, n, bool(complete.value), walked[:n].copy(), kept[:n].copy(),
                hooks[:n].copy(), jumps[:n].copy(), per[:n].copy(), total.value)

    # ---- greedy weighted matching: mate[v] = the partner of v in the matching a serial loop over ascending MKEY gives
    def match_graph(self, row_ptr, col_idx, val):
        """The handle Engine.matching needs (match.MatchGraph), from the CSR arrays of a square matrix whose float32
        values are the weights."""
        from .match import MatchGraph   # (match.py imports this module)
        return self._graph(MatchGraph, row_ptr, col_idx, val)

    def matching(self, G, mate, heavy=1, seed=1, in_match=None, edge_u=None, edge_v=None, weight=None, max_rounds=4096):
        """-> (pairs, rounds, complete, walked, kept, matched, ns, total_ns); per round: the length of the edge list at
        its start, the edges whose ends were both free, the edges matched, device ns.  mate: an int32 vector of >= rows
        elements; in_match, edge_u, edge_v, weight: None or vectors of >= M = G.edges elements.  heavy = 1: the heaviest
        edges first; seed != 0 breaks ties by mix32(e ^ seed), seed = 0 by edge id (on equal weights that costs one round
        per pair in places).  A run has at most rows // 2 + 1 rounds; one cut short leaves a valid matching that is not
        maximal."""
        pairs, rounds, complete, total = C.c_int64(), C.c_int32(), C.c_int32(), C.c_uint64()
        cap = max(int(max_rounds), 1)
        (walked, kept, matched, per), ptrs = _outs(cap, np.int64, np.int64, np.int64, np.uint64)
        h = lambda v: None if v is None else v.h   # noqa: E731
        self._chk(abi.load().sh_match(self.h, G.h, mate.h, h(in_match), h(edge_u), h(edge_v), h(weight), heavy,
                                      int(seed) & 0xFFFFFFFF, max_rounds, C.byref(pairs), C.byref(rounds), C.byref(complete),
                                      *ptrs, C.byref(total)))
        n = rounds.value
        return (pairs.value, n, bool(complete.value), walked[:n].copy(), kept[:n].copy(), matched[:n].copy(), per[:n].copy(),
                total.value)

    # ---- reverse Cuthill-McKee: perm[k] = the vertex at new position k, in the order a serial loop with fixed ties gives
    def rcm_graph(self, row_ptr, col_idx, val):
        """The handle Engine.rcm_order needs (rcm.RcmGraph), from the CSR arrays of a square matrix."""
        from .rcm import RcmGraph   # (rcm.py imports this module)
        return self._graph(RcmGraph, row_ptr, col_idx, val)

    def rcm_order(self, G, perm, pos=None, level=None, sweeps=8, reverse=1, max_steps=None):
        """-> (components, sweeps_run, steps, complete, bandwidth_before, bandwidth_after, profile_before, profile_after,
        kinds, sizes, edges, ns, total_ns); per step (one level of one breadth-first search): 0 for a root search and 1
        for the numbering, the level's width, the sum of its list lengths, device ns.  perm: an int32 vector of >= rows
        elements (A[perm][:, perm] is the reordered matrix); pos, level: None or such vectors.  sweeps: the searches
        George and Liu's root finder may add to the first one, 0 for the first vertex of the walk as the root;
        reverse = 0 gives the Cuthill-McKee order itself.  max_steps = None: min((sweeps + 2) * rows + 1, 2^20); a run
        cut short has complete = False, -1 in the rest of perm and -1 for both values after."""
        if max_steps is None:
            max_steps = min((int(sweeps) + 2) * G.n + 1, 1 << 20)
        components, sweeps_run, steps, complete, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        bw0, bw1, prof0, prof1 = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        cap = max(int(max_steps), 1)
        (kinds, sizes, edges, per), ptrs = _outs(cap, np.int32, np.int64, np.int64, np.uint64)
        h = lambda v: None if v is None else v.h   # noqa: E731
        self._chk(abi.load().sh_rcm(self.h, G.h, perm.h, h(pos), h(level), sweeps, reverse, max_steps, C.byref(components),
                                    C.byref(sweeps_run), C.byref(steps), C.byref(complete), C.byref(bw0), C.byref(bw1),
                                    C.byref(prof0), C.byref(prof1), *ptrs, C.byref(total)))
        n = steps.value
        return (components.value, sweeps_run.value, n, bool(complete.value), bw0.value, bw1.value, prof0.value, prof1.value,
                kinds[:n].copy(), sizes[:n].copy(), edges[:n].copy(), per[:n].copy(), total.value)

    # ---- betweenness centrality: bc[v] = the sum over the sources s != v of delta_s(v), float64, every sum in one fixed order
    def bc_graph(self, row_ptr, col_idx, val):
        """The handle Engine.betweenness needs (bc.BcGraph), from the CSR arrays of a square matrix."""
        from .bc import BcGraph   # (bc.py imports this module)
        return self._graph(BcGraph, row_ptr, col_idx, val)

    def betweenness(self, G, sources, bc, accumulate=0, sigma=None, level=None):
        """-> (steps, depths, reached, sigma_max, edges, ns, total_ns); per source: the last level that holds a vertex, the
        vertices reached (the source included), the largest path count (float64: exact below 2^53, inf once it has
        overflowed), the out-list entries walked forward, device ns.  sources: int32 vertex indices, taken in the order
        given.  bc: a vector of >= 2 * rows 4-byte elements (rows float64 scores; download(np.uint32, 2 * rows).view(np.float64) reads them);
        accumulate = 1 adds to what it holds.  sigma: None or such a vector, level: None or an int32 vector of >= rows
        elements; both get the last source's values."""
        sources = np.ascontiguousarray(sources, np.int32)
        n = len(sources)
        steps, total = C.c_int64(), C.c_uint64()
        (depths, reached, smax, edges, per), ptrs = _outs(max(n, 1), np.int32, np.int64, np.float64, np.int64, np.uint64)
        h = lambda v: None if v is None else v.h   # noqa: E731
        self._chk(abi.load().sh_bc(self.h, G.h, _ptr(sources) if n else None, n, bc.h, accumulate, h(sigma), h(level),
                                   C.byref(steps), *ptrs, C.byref(total)))
        return steps.value, depths[:n].copy(), reached[:n].copy(), smax[:n].copy(), edges[:n].copy(), per[:n].copy(), total.value

    # ---- sparse triangular solve: x = T^-1 b by level sets, float64, every sum in one fixed order
    def trsv_graph(self, row_ptr, col_idx, val, uplo=0, unit=0):
        """The handle Engine.trsv needs (trsv.TrsvGraph), from the CSR arrays of a square matrix: its lower (uplo = 0) or
        upper (1) triangle; unit = 1 takes the diagonal as one and ignores stored diagonal entries.  An ILU(0) factor kept
        in one matrix gives two handles: (uplo=0, unit=1) and (uplo=1, unit=0)."""
        from .trsv import TrsvGraph   # (trsv.py imports this module)
        return self._graph(TrsvGraph, row_ptr, col_idx, val, uplo, unit)

    def trsv(self, G, b, x, f32=0, thin=None):
        """-> (launches, runs, levels_in_runs, total_ns): the launches of the call, how many of them were runs of thin
        levels inside one workgroup, the levels those held, device ns.  b, x: vectors of >= 2 * rows 4-byte elements
        (rows float64, 8-byte aligned), or with f32 = 1 of >= rows float32; x may be b.  thin: consecutive levels of at
        most `thin` rows share a launch (0: one launch per level; None: the default, trsv.TRSV_THIN).  x does not depend
        on thin."""
        launches, runs, in_runs, total = C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64()
        self._chk(abi.load().sh_trsv(self.h, G.h, b.h, x.h, f32, -1 if thin is None else int(thin), C.byref(launches),
                                     C.byref(runs), C.byref(in_runs), C.byref(total)))
        return launches.value, runs.value, in_runs.value, total.value

    # ---- incomplete LU factorisation without fill by level sets, float64, one fixed order
    def ilu0_graph(self, row_ptr, col_idx):
        """The handle Engine.ilu0 needs (ilu0.Ilu0Graph), from the CSR pattern of a square matrix alone: no values."""
        from .ilu0 import Ilu0Graph   # (ilu0.py imports this module)
        row_ptr, col_idx, _ = _csr_args(row_ptr, col_idx, col_idx)
        h = C.c_void_p()
        self._chk(abi.load().sh_ilu0_graph_create(self.h, len(row_ptr) - 1, len(col_idx), _ptr(row_ptr), _ptr(col_idx), C.byref(h)))
        return Ilu0Graph(self, h, len(row_ptr) - 1)

    def ilu0(self, G, val, lu, f32=1, thin=None):
        """-> (launches, runs, levels_in_runs, zero_pivots, first_zero, total_ns): the launches of the call, how many of
        them were runs of thin levels inside one workgroup, the levels those held, the rows whose pivot == 0.0 (a missing
        diagonal counts, a NaN does not), the smallest of them or -1, device ns.  val: a float32 vector of >= nnz elements
        in the order of the entries; lu: >= nnz float32 (f32 = 1; may be val), or >= 2 * nnz 4-byte elements (nnz float64,
        8-byte aligned).  lu[p] = the factor's value at the first entry of its (row, column) group, +0.0 elsewhere: with
        the handle's row_ptr / col_idx it is L (trsv_graph(uplo=0, unit=1)) and U (uplo=1, unit=0) in one matrix.  thin:
        as Engine.trsv's.  lu does not depend on thin."""
        launches, runs, in_runs, zero, first, total = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_uint64()
        self._chk(abi.load().sh_ilu0(self.h, G.h, val.h, lu.h, f32, -1 if thin is None else int(thin), C.byref(launches),
                                     C.byref(runs), C.byref(in_runs), C.byref(zero), C.byref(first), C.byref(total)))
        return launches.value, runs.value, in_runs.value, zero.value, first.value, total.value

    # ---- several vectors per launch (element i of vector j at i * width + j; the matrix uploaded with plan=1)
    def spmm(self, semiring, A, X, Y, alpha, beta, Out, width, timed=False):
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        ns = C.c_uint64()
        self._chk(abi.load().sh_spmm(self.h, semiring, A.h, width, X.h, None if Y is None else Y.h, _ptr(a), _ptr(b),
                                     Out.h, C.byref(ns) if timed else None))
        return ns.value if timed else None

    def iterate_multi(self, semiring, A, X, Y0, scratch, alpha, beta, width, delta=1e-4, max_iters=10000):
        """-> (launches, iters_of_column, converged_of_column, ns_per_launch, total_ns)"""
        dt = elem_dtype(semiring)
        a, b = np.array([alpha], dt), np.array([beta], dt)
        launches, total = C.c_int32(), C.c_uint64()
        cap = max(int(width), 1)   # (a width the engine refuses still gets buffers it could not overrun)
        iters, conv = (C.c_int32 * cap)(), (C.c_int32 * cap)()
        per = (C.c_uint64 * max(max_iters, 1))()
        self._chk(abi.load().sh_iterate_multi(self.h, semiring, A.h, width, X.h, None if Y0 is None else Y0.h, scratch.h,
                                              _ptr(a), _ptr(b), delta, max_iters, C.byref(launches), iters, conv, per,
                                              C.byref(total)))
        return launches.value, list(iters[:width]), [bool(c) for c in conv[:width]], list(per[:launches.value]), total.value

    # ---- (or,and) on packed bits: 32 * words sources, word w of vertex v at v * words + w, source s = bit s % 32 of word s // 32
    def bits_spmv(self, A, X, Y, alpha, beta, Out, words, timed=False):
        a, b = np.array([alpha], np.int32), np.array([beta], np.int32)
        ns = C.c_uint64()
        self._chk(abi.load().sh_bits_spmv(self.h, A.h, words, X.h, None if Y is None else Y.h, _ptr(a), _ptr(b), Out.h,
                                          C.byref(ns) if timed else None))
        return ns.value if timed else None

    def bits_iterate(self, A, X, Y0, scratch, alpha, beta, words, max_iters=10000, counts=False):
        """-> (launches, iters_of_source, converged_of_source, ns_per_launch, total_ns[, newly_set (launches, 32 * words)])"""
        a, b = np.array([alpha], np.int32), np.array([beta], np.int32)
        launches, total = C.c_int32(), C.c_uint64()
        n_src = 32 * max(int(words), 1)   # (a `words` the engine refuses still gets buffers it could not overrun)
        iters, conv = (C.c_int32 * n_src)(), (C.c_int32 * n_src)()
        per = (C.c_uint64 * max(max_iters, 1))()
        newly = np.zeros((max(max_iters, 0), n_src), np.uint32) if counts else None
        self._chk(abi.load().sh_bits_iterate(self.h, A.h, words, X.h, None if Y0 is None else Y0.h, scratch.h, _ptr(a), _ptr(b),
                                             max_iters, C.byref(launches), iters, conv,
                                             newly.ctypes.data_as(C.POINTER(C.c_uint32)) if counts else None, per, C.byref(total)))
        n_src = 32 * int(words)
        res = (launches.value, list(iters[:n_src]), [bool(c) for c in conv[:n_src]], list(per[:launches.value]), total.value)
        return res + (newly[:launches.value, :n_src].copy(),) if counts else res

    def bits_from_column(self, v, n, words, source, B):
        self._chk(abi.load().sh_bits_from_column(self.h, v.h, n, words, source, B.h))

    def bits_to_column(self, B, n, words, source, v):
        self._chk(abi.load().sh_bits_to_column(self.h, B.h, n, words, source, v.h))
