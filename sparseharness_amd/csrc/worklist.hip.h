// worklist.hip.h -- what the worklist algorithms share (frontier.hip.h, bfs.hip.h, sssp.hip.h, ..., core.hip.h, truss.hip.h): list cursors, the cutting
// of long lists into pieces, the folds (over a wave, over a workgroup, over a launch's per-workgroup parts), the gate of a
// closing kernel, the jump pass, the two traversal skeletons and the kernels that build a graph handle.
//
// Folds: wl_wave_fold<OP> and wl_block_fold<OP> with OP one of WlSum, WlMin, WlMax, on 32- and 64-bit unsigned words;
// wl_block_part writes a workgroup's WlPart and wl_sum_parts folds a launch's.  An algorithm writes no fold of its own:
// a part of another layout (TrussPart, TriPart, RcmFin) or two part arrays at once are a strided loop of the kernel's
// and wl_block_fold per word.  What is not a fold stays with its kernel: scans and rankings (rcm_block_scan, rcm_tile,
// frontier_detect), the arg-max over a pair that fits no word (scc_block_best), a semiring-typed wave reduction
// (fr_wave_reduce) and the double sum of sssp_weight_sum, whose order of additions is part of its result.
//
// Work distribution: every kernel runs a fixed grid whose waves stride over a device-side list length (the host does
// not know it).  A wave takes 64 list entries at a time: lists of up to SHORT entries one lane each, longer ones the
// whole wave one after the other, and those above PIECE entries are cut into pieces of that size which go through a
// list of their own (built by whoever appended the entry: wl_push_pieces), one wave per piece.  wl_expand is that
// traversal for a push along the lists of a worklist's entries, wl_rows_min for a pass over all rows that looks for the
// smallest matching in-neighbour.  The loops whose bodies do not fit either (a reduction in a semiring type, an early
// exit, a two-pass reservation, a prefix scan, a list split) stay with their kernels and use the helpers only: a
// skeleton wide enough to serve them would branch on its caller.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace sh {

constexpr int WL_BS = 256;   // threads of a workgroup of every worklist kernel

struct WlPiece { uint32_t id, off; };   // whose list (a vertex, a row, or a slot of a list of rows), first entry of the piece
// Per workgroup of a traversal launch: its sums (no atomics on one address: thousands of waves adding to one word
// retire about 6 ns apart, see frontier_detect).
struct WlPart { uint32_t a, b, c, pad; };

__device__ __forceinline__ int wl_lane() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ int64_t wl_wave() { return (int64_t)blockIdx.x * (WL_BS / 64) + (threadIdx.x >> 6); }
__device__ __forceinline__ int64_t wl_waves() { return (int64_t)gridDim.x * (WL_BS / 64); }

__device__ __forceinline__ uint32_t wl_add(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One atomic per wave for a list cursor: the first wanting lane adds the count, every wanting lane gets its place.
// (Call from wave-uniform control flow only.)
__device__ __forceinline__ uint32_t wl_wave_append(uint32_t *cursor, bool want, int lane) {
  const uint64_t m = __ballot(want);
  if (m == 0) return 0;
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint32_t base = 0;
  if (lane == leader) base = wl_add(cursor, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
// A place in a list for every lane that gets here together (any control flow: the ballot covers the active lanes, the
// lowest of them adds for all and readfirstlane hands its answer round); one add per lane serialises on the one address.
__device__ __forceinline__ uint32_t wl_append_here(uint32_t *cursor) {
  const uint64_t here = __ballot(1);
  const int lane = wl_lane();
  uint32_t first = 0;
  if (lane == __ffsll((unsigned long long)here) - 1) first = wl_add(cursor, (uint32_t)__popcll(here));
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)first) + (uint32_t)__popcll(here & ((1ull << lane) - 1ull));
}
// Relaxed agent-scope one-liners: a load that goes to the L2, where the atomics meet, and the two unsigned atomics that
// only ever move a word one way (-> the word as it was).
template <class T>
__device__ __forceinline__ T wl_load(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t wl_umin(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t wl_umax(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The lanes of a wave meet, and what they stored to the wave's LDS words before is what they load after.
__device__ __forceinline__ void wl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- folds.  The operations are associative and commutative on integers: no result depends on who folds first.
struct WlSum { template <class T> __device__ static T of(T a, T b) { return a + b; } };
struct WlMin { template <class T> __device__ static T of(T a, T b) { return min(a, b); } };
struct WlMax { template <class T> __device__ static T of(T a, T b) { return max(a, b); } };
// The wave's word -> every lane (wave-uniform control flow only).
template <class OP, class T>
__device__ __forceinline__ T wl_wave_fold(T v) {
  for (int o = 32; o > 0; o >>= 1) v = OP::of(v, (T)__shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wl_wave_sum(uint32_t v) { return wl_wave_fold<WlSum>(v); }
__device__ __forceinline__ uint32_t wl_wave_min(uint32_t v) { return wl_wave_fold<WlMin>(v); }
// The workgroup's word -> EVERY thread: shuffles inside a wave, one LDS word per wave.  CONVERGENT CONTROL FLOW ONLY:
// every thread of the workgroup calls it, all of them together (it holds barriers).  A kernel may call it as often as it
// likes: the array below is one array however often this is inlined, so the first barrier keeps a call from writing
// the words that a thread is still reading for the call before.
template <class OP, class T>
__device__ __forceinline__ T wl_block_fold(T v) {
  __shared__ T s_w[WL_BS / 64];
  v = wl_wave_fold<OP>(v);
  __syncthreads();
  if (wl_lane() == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_w[0];
  for (int w = 1; w < WL_BS / 64; w++) v = OP::of(v, s_w[w]);
  return v;
}
// A word of thread 0 -> every thread of the workgroup (one LDS word, one barrier; convergent control flow only, and once
// per kernel: nothing keeps a second call from overwriting the word under a late reader).  THE GATE OF A CLOSING KERNEL,
// `if (!wl_from_thread0(ctl->step == s)) return;`, needs it: thread 0 stores the next step further down, so a wave that
// read the step for itself, late, could leave before a barrier at which its siblings wait.
__device__ __forceinline__ uint32_t wl_from_thread0(uint32_t v) {
  __shared__ uint32_t s_v;
  if (threadIdx.x == 0) s_v = v;
  __syncthreads();
  return s_v;
}
// The pieces of a list of `len` entries join piece list `list` (nothing when it is no longer than PIECE).  A piece list
// over lists that hold E entries in all needs E / (PIECE / 2) + 1 places: sum of ceil(len / PIECE) over len > PIECE.
template <int PIECE>
__device__ __forceinline__ void wl_push_pieces(uint32_t *cursor, uint32_t id, uint32_t len, WlPiece *__restrict__ list) {
  if (len > (uint32_t)PIECE) {
    const uint32_t np = (len + PIECE - 1) / PIECE;
    const uint32_t b = wl_add(cursor, np);
    for (uint32_t j = 0; j < np; j++) list[b + j] = WlPiece{id, j * PIECE};
  }
}
// The workgroup's WlPart -> EVERY thread: a is summed, b folded by OPB and c by OPC (WlSum or WlMax: 0 is the neutral
// word of either; WlNone: the part has no c, the word stays 0).  CONVERGENT CONTROL FLOW ONLY, and ONE barrier for all
// the words, none ahead of them: parts are written by every traversal launch and folded once per round, and a
// round-heavy run is bound by just these latencies.  So, unlike wl_block_fold and like wl_from_thread0, ONCE PER KERNEL
// (the words are its own, not wl_block_fold's): a kernel has one part to write, a closing kernel one array of them to
// fold -- wl_block_part and wl_sum_parts are its only callers, and a kernel calls one of them on one path.
struct WlNone {};
template <class OPB, class OPC>
__device__ __forceinline__ WlPart wl_block_fold_part(uint32_t a, uint32_t b, uint32_t c) {
  constexpr bool HAS_C = !std::is_same<OPC, WlNone>::value;
  __shared__ uint32_t s_w[HAS_C ? 3 : 2][WL_BS / 64];
  const int wv = (int)(threadIdx.x >> 6);
  a = wl_wave_fold<WlSum>(a);
  b = wl_wave_fold<OPB>(b);
  if constexpr (HAS_C) c = wl_wave_fold<OPC>(c);
  if (wl_lane() == 0) {
    s_w[0][wv] = a; s_w[1][wv] = b;
    if constexpr (HAS_C) s_w[2][wv] = c;
  }
  __syncthreads();
  WlPart t{s_w[0][0], s_w[1][0], 0u, 0u};
  if constexpr (HAS_C) t.c = s_w[2][0];
  for (int w = 1; w < WL_BS / 64; w++) {
    t.a += s_w[0][w]; t.b = OPB::of(t.b, s_w[1][w]);
    if constexpr (HAS_C) t.c = OPC::of(t.c, s_w[2][w]);
  }
  return t;
}
// The workgroup's words -> its WlPart (once per kernel: it has one part).
template <class OPB = WlSum, class OPC = WlNone>
__device__ __forceinline__ void wl_block_part(WlPart *__restrict__ part, uint32_t a, uint32_t b, uint32_t c = 0u) {
  const WlPart t = wl_block_fold_part<OPB, OPC>(a, b, c);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}
// A launch's WlParts folded the same way, by one workgroup -> every thread (once per kernel).
template <class OPB = WlSum, class OPC = WlNone>
__device__ __forceinline__ WlPart wl_sum_parts(const WlPart *__restrict__ part, int nparts) {
  uint32_t a = 0, b = 0, c = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) {
    a += part[i].a; b = OPB::of(b, part[i].b);
    if constexpr (!std::is_same<OPC, WlNone>::value) c = OPC::of(c, part[i].c);
  }
  return wl_block_fold_part<OPB, OPC>(a, b, c);
}

// The jump pass of a parent forest whose pointers only go towards the root (wcc.hip.h, msf.hip.h), launch i of a
// round's sweeps, over all rows: p[v] = p[p[v]] until p[v] is a root as this lane sees it, `jumps` times at most.  No
// hook runs beside it, so p[v] is written by the lane of v alone; what it reads of others is a pointer they hold now
// or held before, an ancestor either way.  The pointers the workgroup changed are added to jpart[].a (launch 0 of the
// round stores), and moved[i] says whether anybody changed one (wl_block_fold's contract).
__device__ __forceinline__ void wl_jump(int i, int jumps, int32_t rows, uint32_t *p, WlPart *__restrict__ jpart, uint32_t *moved_flags) {
  uint32_t moved = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    uint32_t q = p[v];
    for (int h = 0; h < jumps; h++) {
      const uint32_t up = p[q];
      if (up == q) break;
      p[v] = q = up;
      moved++;
    }
  }
  moved = wl_block_fold<WlSum>(moved);
  if (threadIdx.x == 0) {
    jpart[blockIdx.x].a = i == 0 ? moved : jpart[blockIdx.x].a + moved;   // (this thread alone, launch after launch)
    if (moved) moved_flags[i] = 1u;                                        // (whoever stores it stores the same word)
  }
}

// The push traversal: for every v of list[0, n) the entries [ptr[v], ptr[v + 1]), lists above PIECE entries through
// pieces[0, np) instead.  visit(v, true) runs once per valid list entry and returns a 32-bit word that the skeleton
// carries to the lanes that walk v's list; a piece reads it again as visit(v, false), which must do nothing else.
// edge(j, carried) runs once per entry j.  -> the lane's sum of list lengths.
template <int SHORT, int PIECE, class Visit, class Edge>
__device__ __forceinline__ uint32_t wl_expand(const uint32_t *__restrict__ list, int64_t n, const WlPiece *__restrict__ pieces,
                                              int64_t np, const int32_t *__restrict__ ptr, Visit visit, Edge edge) {
  const int lane = wl_lane();
  uint32_t looked = 0;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const int32_t v = valid ? (int32_t)list[base + lane] : 0;
    const int32_t s = valid ? ptr[v] : 0;
    const int32_t len = valid ? ptr[v + 1] - s : 0;
    const uint32_t w = valid ? visit(v, true) : 0u;
    looked += (uint32_t)len;
    if (len <= SHORT)
      for (int32_t j = 0; j < len; j++) edge(s + j, w);
    uint64_t m = __ballot(len > SHORT && len <= PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const uint32_t wb = (uint32_t)__shfl((int)w, src);
      for (int32_t j = lane; j < lb; j += 64) edge(sb + j, wb);
    }
  }
  for (int64_t q = wl_wave(); q < np; q += wl_waves()) {   // a hub's list: one wave per piece
    const WlPiece pc = pieces[q];
    const int32_t s = ptr[pc.id] + (int32_t)pc.off;
    const int32_t e = min(s + PIECE, ptr[pc.id + 1]);
    const uint32_t w = visit((int32_t)pc.id, false);
    for (int32_t j = s + lane; j < e; j += 64) edge(j, w);
  }
  return looked;
}

// The row pass: out[r] = the smallest in_col[j] over the entries j of row r with hit(j, want), for every row with
// open(r, &want) (whether row r takes part, and its wanted word).  The host fills `out` with -1 first; pieces of rows
// above PIECE entries (rpieces: a static list) meet in out[r] by an UNSIGNED atomic min, under which -1 (no candidate
// yet) is the largest word.
template <int SHORT, int PIECE, class Open, class Hit>
__device__ __forceinline__ void wl_rows_min(int32_t rows, const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_col,
                                            const WlPiece *__restrict__ rpieces, int32_t n_rpieces, int32_t *out, Open open, Hit hit) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const int64_t r = base + lane;
    uint32_t want = 0;
    const bool on = r < rows && open((int32_t)r, &want);
    const int32_t s = on ? in_ptr[r] : 0;
    const int32_t len = on ? in_ptr[r + 1] - s : 0;
    uint32_t best = 0xFFFFFFFFu;
    if (len <= SHORT)
      for (int32_t j = s; j < s + len; j++)
        if (hit(j, want)) best = min(best, (uint32_t)in_col[j]);
    uint64_t m = __ballot(len > SHORT && len <= PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const uint32_t wb = (uint32_t)__shfl((int)want, src);
      uint32_t mine = 0xFFFFFFFFu;
      for (int32_t j = sb + lane; j < sb + lb; j += 64)
        if (hit(j, wb)) mine = min(mine, (uint32_t)in_col[j]);
      mine = wl_wave_min(mine);
      if (lane == src) best = mine;
    }
    if (len > 0 && len <= PIECE) out[r] = (int32_t)best;
  }
  for (int64_t i = wl_wave(); i < n_rpieces; i += wl_waves()) {
    const WlPiece pc = rpieces[i];
    const int32_t r = (int32_t)pc.id;
    uint32_t want = 0;
    if (!open(r, &want)) continue;
    const int32_t s = in_ptr[r] + (int32_t)pc.off;
    const int32_t e = min(s + PIECE, in_ptr[r + 1]);
    uint32_t mine = 0xFFFFFFFFu;
    for (int32_t j = s + lane; j < e; j += 64)
      if (hit(j, want)) mine = min(mine, (uint32_t)in_col[j]);
    mine = wl_wave_min(mine);
    if (lane == 0 && mine != 0xFFFFFFFFu)
      (void)__hip_atomic_fetch_min((uint32_t *)&out[r], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- building a handle (once): the entries that are edges, compacted in stored order; the static pieces of long rows;
// the transpose (column histogram, exclusive scan by rocPRIM in plan_gpu.hip, scatter through per-column cursors)
// flag[j] = entry j is an edge: KEEP::value(its value word) and a column inside the matrix (flag[nnz] = 0 closes the scan)
template <class KEEP>
__global__ __launch_bounds__(WL_BS) void wl_edge_flag(const int32_t *__restrict__ col_idx, const uint32_t *__restrict__ val,
                                                      int64_t nnz, int32_t cols, uint32_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz) flag[j] = (KEEP::value(val[j]) && (uint32_t)col_idx[j] < (uint32_t)cols) ? 1u : 0u;
  else if (j == nnz) flag[j] = 0u;
}
// pos = exclusive scan of flag: edge j goes to in_col[pos[j]] and, where weights are kept (in_w != NULL), its |a| to in_w[pos[j]]
__global__ __launch_bounds__(WL_BS) void wl_edge_compact(const int32_t *__restrict__ col_idx, const uint32_t *__restrict__ val,
                                                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                         int64_t nnz, int32_t *__restrict__ in_col, uint32_t *__restrict__ in_w) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz && flag[j]) {
    in_col[pos[j]] = col_idx[j];
    if (in_w) in_w[pos[j]] = val[j] & 0x7FFFFFFFu;
  }
}
__global__ __launch_bounds__(WL_BS) void wl_row_starts(const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ pos,
                                                       int64_t rows, int32_t *__restrict__ in_ptr) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (r <= rows) in_ptr[r] = (int32_t)pos[row_ptr[r]];
}
template <int PIECE>
__global__ __launch_bounds__(WL_BS) void wl_row_pieces(const int32_t *__restrict__ in_ptr, int64_t rows, uint32_t *cursor,
                                                       WlPiece *__restrict__ rpieces) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (r < rows) wl_push_pieces<PIECE>(cursor, (uint32_t)r, (uint32_t)(in_ptr[r + 1] - in_ptr[r]), rpieces);
}
__global__ __launch_bounds__(WL_BS) void wl_col_hist(const int32_t *__restrict__ col_idx, int64_t nnz, int32_t cols,
                                                     uint32_t *__restrict__ cnt) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz) {
    const int32_t c = col_idx[j];
    if ((uint32_t)c < (uint32_t)cols) wl_add(&cnt[c], 1u);
  }
}
// Entry j of row r goes to the list of its column, with its weight where there are weights (w != NULL).  (The row of
// entry j by bisection of row_ptr: one-off work, and a hub row is spread over its entries' lanes.  The column is
// checked: sh_frontier_create passes arrays that are not compacted.)
__global__ __launch_bounds__(WL_BS) void wl_transpose_scatter(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                              const uint32_t *__restrict__ w, int64_t nnz, int32_t rows, int32_t cols,
                                                              uint32_t *__restrict__ cursor, int32_t *__restrict__ row_of,
                                                              uint32_t *__restrict__ out_w) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j >= nnz) return;
  const int32_t c = col_idx[j];
  if ((uint32_t)c >= (uint32_t)cols) return;
  int32_t lo = 0, hi = rows;   // last r with row_ptr[r] <= j
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if ((int64_t)row_ptr[mid] <= j) lo = mid; else hi = mid;
  }
  const uint32_t at = wl_add(&cursor[c], 1u);
  row_of[at] = lo;
  if (w) out_w[at] = w[j];
}

// ---- building the handle of sh_tri (once): the simple undirected graph under the entries, oriented, every forward
// list strictly ascending.  An edge {u, v} is one 64-bit key (first << bits | second), `bits` = the bits of rows - 1, so
// that a radix sort looks at 2 * bits bits only (the sorts and scans are rocPRIM's, in plan_gpu.hip).
// The row of entry j: the last r with row_ptr[r] <= j (one-off work, as in wl_transpose_scatter).
__device__ __forceinline__ int32_t wl_row_of(const int32_t *__restrict__ row_ptr, int32_t rows, int64_t j) {
  int32_t lo = 0, hi = rows;
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if ((int64_t)row_ptr[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}
// flag[j] = entry j counts (wl_edge_flag's rule) and is no self-loop (flag[nnz] = 0 closes the scan)
template <class KEEP>
__global__ __launch_bounds__(WL_BS) void wl_und_flag(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                     const uint32_t *__restrict__ val, int64_t nnz, int32_t rows,
                                                     uint32_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz) {
    const int32_t c = col_idx[j];
    flag[j] = (KEEP::value(val[j]) && (uint32_t)c < (uint32_t)rows && c != wl_row_of(row_ptr, rows, j)) ? 1u : 0u;
  } else if (j == nnz) flag[j] = 0u;
}
// pos = exclusive scan of flag: survivor j -> key[pos[j]] = (min(r, c) << bits | max(r, c))
__global__ __launch_bounds__(WL_BS) void wl_und_keys(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                     const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                     int64_t nnz, int32_t rows, int bits, uint64_t *__restrict__ key) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz && flag[j]) {
    const uint32_t r = (uint32_t)wl_row_of(row_ptr, rows, j), c = (uint32_t)col_idx[j];
    key[pos[j]] = ((uint64_t)min(r, c) << bits) | (uint64_t)max(r, c);
  }
}
// head[i] = sorted key i is the first of its run: one per edge of the simple graph (head[n] = 0 closes the scan)
__global__ __launch_bounds__(WL_BS) void wl_run_heads(const uint64_t *__restrict__ key, int64_t n, uint32_t *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
  else if (i == n) head[i] = 0u;
}
// deg as a histogram over both ends of every edge (deg zeroed by the host)
__global__ __launch_bounds__(WL_BS) void wl_und_degrees(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head, int64_t n,
                                                        int bits, uint32_t *__restrict__ deg) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    wl_add(&deg[key[i] >> bits], 1u);
    wl_add(&deg[key[i] & ((1ull << bits) - 1ull)], 1u);
  }
}
// Edge i of the simple graph (pos = exclusive scan of head) -> okey[pos[i]] = (src << bits | dst).  order 0: from the
// smaller index to the larger; order 1: from the smaller (deg, index) pair to the larger.
__global__ __launch_bounds__(WL_BS) void wl_orient(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                   const uint32_t *__restrict__ pos, int64_t n, int bits, int32_t order,
                                                   const uint32_t *__restrict__ deg, uint64_t *__restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    const uint64_t u = key[i] >> bits, v = key[i] & ((1ull << bits) - 1ull);   // u < v
    const bool swap = order == 1 && deg[v] < deg[u];                           // (equal degrees: the smaller index first)
    okey[pos[i]] = swap ? ((v << bits) | u) : ((u << bits) | v);
  }
}
// Edge i of the simple graph (pos = exclusive scan of head), both ways, for the symmetric lists of sh_core_graph:
// okey[2 * pos[i]] = (u << bits | v) and okey[2 * pos[i] + 1] = (v << bits | u)
__global__ __launch_bounds__(WL_BS) void wl_both_ways(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                      const uint32_t *__restrict__ pos, int64_t n, int bits,
                                                      uint64_t *__restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    const uint64_t u = key[i] >> bits, v = key[i] & ((1ull << bits) - 1ull);
    okey[2 * (int64_t)pos[i]] = (u << bits) | v;
    okey[2 * (int64_t)pos[i] + 1] = (v << bits) | u;
  }
}
// Edge i of the simple graph (pos = exclusive scan of head) is edge pos[i] of sh_truss_graph -- the keys are sorted, so the
// ids run in the order of the pairs (u, v), u < v: eu[pos[i]] = u, ev[pos[i]] = v
__global__ __launch_bounds__(WL_BS) void wl_edge_ends(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                      const uint32_t *__restrict__ pos, int64_t n, int bits,
                                                      int32_t *__restrict__ eu, int32_t *__restrict__ ev) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    eu[pos[i]] = (int32_t)(key[i] >> bits);
    ev[pos[i]] = (int32_t)(key[i] & ((1ull << bits) - 1ull));
  }
}
// eid[j] = the edge that entry j of the symmetric lists ptr / col (n entries) stands for: the row of j by bisection of ptr
// (wl_row_of), the pair (min, max) by bisection of the m edges eu / ev, which hold it (one-off work)
__global__ __launch_bounds__(WL_BS) void wl_edge_ids(const int32_t *__restrict__ ptr, const int32_t *__restrict__ col, int64_t n,
                                                     int32_t rows, const int32_t *__restrict__ eu, const int32_t *__restrict__ ev,
                                                     int64_t m, int32_t *__restrict__ eid) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j >= n) return;
  const int32_t r = wl_row_of(ptr, rows, j), c = col[j];
  const int32_t a = min(r, c), b = max(r, c);
  int64_t lo = 0, hi = m;   // the first edge that is not below (a, b)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (eu[mid] < a || (eu[mid] == a && ev[mid] < b)) lo = mid + 1; else hi = mid;
  }
  eid[j] = (int32_t)min(lo, m - 1);
}
// From the sorted oriented keys: fwd_col, and fwd_ptr[r] = the first key of a source >= r (r in [0, rows]; a bisection
// over m keys per row)
__global__ __launch_bounds__(WL_BS) void wl_forward_lists(const uint64_t *__restrict__ okey, int64_t m, int64_t rows, int bits,
                                                          int32_t *__restrict__ fwd_ptr, int32_t *__restrict__ fwd_col) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < m) fwd_col[i] = (int32_t)(okey[i] & ((1ull << bits) - 1ull));
  if (i <= rows) {
    int64_t lo = 0, hi = m;   // the first key with (key >> bits) >= i
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if ((int64_t)(okey[mid] >> bits) < i) lo = mid + 1; else hi = mid;
    }
    fwd_ptr[i] = (int32_t)lo;
  }
}
// *out = the longest list of ptr (a fixed grid: one atomic per wave of it; *out zeroed by the host)
__global__ __launch_bounds__(WL_BS) void wl_max_len(const int32_t *__restrict__ ptr, int64_t rows, uint32_t *out) {
  uint32_t best = 0;
  for (int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x; r < rows; r += (int64_t)gridDim.x * WL_BS)
    best = max(best, (uint32_t)(ptr[r + 1] - ptr[r]));
  best = wl_wave_fold<WlMax>(best);
  if (wl_lane() == 0 && best) (void)__hip_atomic_fetch_max(out, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace sh
