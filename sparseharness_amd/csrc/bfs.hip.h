// bfs.hip.h -- kernels of sh_bfs_levels: a direction-optimising BFS (Beamer, Asanovic, Patterson: "Direction-optimizing
// breadth-first search", SC 2012) that reports the level of every vertex and, on request, a canonical parent
// (DESIGN.md "6e Direction-optimising BFS").
//
// The graph lives in a layout of its own (sh_bfs_graph): the edge pattern by rows (in_ptr / in_col: the entries of
// row r with a non-zero value and a column inside the matrix, i.e. the edges c -> r, 4 B each) and its transpose
// (out_ptr / out_row: the rows that hold an entry of column c).  Step L assigns level L + 1 from the frontier F_L:
//   bfs_topdown     walks the out-lists of the vertices of a frontier QUEUE; a lane that finds level[r] == -1 claims r
//                   by compare-and-swap, and the winner appends r to the next queue, sets its bit in the next bitmap
//                   and adds r's out-list length to m_{L+1} (what the switching rule looks at);
//   bfs_bottomup    walks the rows; an unvisited row reads its in_col until it meets a column whose bit is set in the
//                   frontier BITMAP, takes level L + 1, sets its bit in the next bitmap and STOPS.  (The semiring
//                   contract forbids that early exit to sh_spmv; "the levels of a BFS" allows it.)
//   bfs_queue_from_bitmap   rebuilds the queue when a top-down step follows a bottom-up one;
//   bfs_decide      closes every step: records what it did, applies the switching rule, clears the consumed bitmap.
// The host does not know a step's direction in advance, so it enqueues for every step the conversion, the top-down and
// the bottom-up launch; each returns at once unless BfsCtl says that this step is running in its direction.  No kernel
// ever waits for another kernel's write: the gate words a kernel reads were written by a launch that ended before it.
// bfs_parents is one row-parallel pass after the traversal (min over the row), so the traversal carries no parent atomics.
//
// Work distribution as worklist.hip.h describes it.  The handle is built by its kernels: wl_edge_flag<BfsKeep>,
// wl_edge_compact, wl_row_starts, wl_row_pieces<BFS_ROW_PIECE>, wl_col_hist, wl_transpose_scatter.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int BFS_SHORT = 8;            // out-lists (top-down) / rows (parent pass) up to this many edges: one lane each
constexpr int BFS_BU_SHORT = 32;        // bottom-up: rows up to this many edges one lane each (the early exit makes a lane's walk short)
constexpr int BFS_OUT_PIECE = 2048;     // out-lists above this are expanded in pieces of this many edges
constexpr int BFS_ROW_PIECE = 4096;     // rows above this are searched in pieces of this many edges (a static list)
constexpr int BFS_BATCH = 32;           // steps enqueued ahead of the host at most (the first batch holds 8)
constexpr int BFS_MAX_BLOCKS = 1024;    // workgroups of a traversal launch at most: one WlPart each
constexpr int BFS_CTL_BYTES = 2048;     // device bytes set aside for BfsCtl
constexpr int BFS_PART_BYTES = 16 * BFS_MAX_BLOCKS;

struct BfsRec {   // what step k of a batch did (read back by the host once per batch)
  int32_t ran, mode, done;
  uint32_t found, edges;
};
// Control block in device memory.  The frontier of step L lives in queue / piece list / bitmap L & 1, the one it
// produces in the other set.
struct BfsCtl {
  uint32_t qcount[2], qpieces[2];   // length of the frontier queue / of its list of long out-list pieces
  int32_t step;                     // the step that runs next (-1 once the search has finished)
  int32_t mode;                     // its direction: 0 top-down, 1 bottom-up
  int32_t have_queue;               // its frontier exists as a queue (not after a bottom-up step)
  int32_t finished;
  uint32_t nsrc, fsize;             // number of sources; size of the frontier of `step`
  BfsRec rec[BFS_BATCH];
};
// The WlPart of a workgroup of a traversal launch.  init: a = out-list lengths of the sources.  top-down: a = edges looked
// at, b = out-list lengths of the vertices claimed.  bottom-up: a = rows that found a parent, b = edges looked at.

struct BfsKeep {   // wl_edge_flag: an entry is an edge when its value word is not zero (and its column is inside the matrix)
  __device__ static bool value(uint32_t v) { return v != 0u; }
};

__device__ __forceinline__ bool bfs_bit(const uint32_t *__restrict__ bm, int32_t v) { return (bm[v >> 5] >> (v & 31)) & 1u; }
__device__ __forceinline__ void bfs_or(uint32_t *p, uint32_t v) {
  (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the search
// level from x0; the sources into queue 0 and bitmap 0 (every word of bitmap 0 is written), their out-list lengths summed.
__global__ __launch_bounds__(WL_BS) void bfs_init(BfsCtl *ctl, int32_t rows, int32_t words, const uint32_t *__restrict__ x0,
                                                   int32_t *__restrict__ level, const int32_t *__restrict__ out_ptr,
                                                   uint32_t *__restrict__ queue, WlPiece *__restrict__ pl, uint32_t *__restrict__ bm,
                                                   WlPart *__restrict__ part) {
  const int lane = wl_lane();
  uint32_t m = 0;
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const int64_t r = base + lane;
    const bool src = r < rows && x0[r] != 0u;
    if (r < rows) level[r] = src ? 0 : -1;
    const uint32_t at = wl_wave_append(&ctl->qcount[0], src, lane);
    if (src) {
      queue[at] = (uint32_t)r;
      const uint32_t len = (uint32_t)(out_ptr[r + 1] - out_ptr[r]);
      wl_push_pieces<BFS_OUT_PIECE>(&ctl->qpieces[0], (uint32_t)r, len, pl);
      m += len;
    }
    const uint64_t sm = __ballot(src);
    const int64_t w = base >> 5;
    if (lane == 0 && w < words) bm[w] = (uint32_t)sm;
    if (lane == 32 && w + 1 < words) bm[w + 1] = (uint32_t)(sm >> 32);
  }
  wl_block_part(part, m, 0u);
}

// r was found unvisited by a top-down lane: the one that wins the compare-and-swap owns it
__device__ __forceinline__ uint32_t bfs_visit(BfsCtl *ctl, int q, int32_t r, int32_t next_level, int32_t *level,
                                              const int32_t *__restrict__ out_ptr, uint32_t *__restrict__ queue,
                                              WlPiece *__restrict__ pl, uint32_t *bm) {
  if (level[r] != -1) return 0;   // (a stale -1 only costs a compare-and-swap that fails; a level never returns to -1)
  int32_t expect = -1;
  if (!__hip_atomic_compare_exchange_strong(&level[r], &expect, next_level, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT))
    return 0;
  queue[wl_append_here(&ctl->qcount[q])] = (uint32_t)r;
  bfs_or(&bm[r >> 5], 1u << (r & 31));
  const uint32_t len = (uint32_t)(out_ptr[r + 1] - out_ptr[r]);
  wl_push_pieces<BFS_OUT_PIECE>(&ctl->qpieces[q], (uint32_t)r, len, pl);
  return len;
}

__global__ __launch_bounds__(WL_BS) void bfs_topdown(BfsCtl *ctl, int L, int32_t *level, const int32_t *__restrict__ out_ptr,
                                                      const int32_t *__restrict__ out_row, const uint32_t *__restrict__ queue,
                                                      const WlPiece *__restrict__ pl, uint32_t *__restrict__ queue_next,
                                                      WlPiece *__restrict__ pl_next, uint32_t *bm_next, WlPart *__restrict__ part) {
  if (ctl->step != L || ctl->mode != 0) return;
  const int p = L & 1, q = p ^ 1;
  uint32_t m_next = 0;
  const uint32_t looked = wl_expand<BFS_SHORT, BFS_OUT_PIECE>(
      queue, ctl->qcount[p], pl, ctl->qpieces[p], out_ptr, [](int32_t, bool) { return 0u; },
      [&](int32_t j, uint32_t) { m_next += bfs_visit(ctl, q, out_row[j], L + 1, level, out_ptr, queue_next, pl_next, bm_next); });
  wl_block_part(part, looked, m_next);
}

// Does [s, e) of in_col hold a column of the frontier?  The whole wave looks, 64 edges at a time, and stops at the first
// group with a hit.  *looked (wave-uniform) grows by the edges of the groups read.
__device__ __forceinline__ bool bfs_wave_search(const int32_t *__restrict__ in_col, const uint32_t *__restrict__ bm, int32_t s, int32_t e,
                                                int lane, uint32_t *looked) {
  for (int32_t j0 = s; j0 < e; j0 += 64) {
    const bool mine = j0 + lane < e && bfs_bit(bm, in_col[j0 + lane]);
    *looked += (uint32_t)min(64, e - j0);
    if (__ballot(mine)) return true;
  }
  return false;
}

__global__ __launch_bounds__(WL_BS) void bfs_bottomup(BfsCtl *ctl, int L, int32_t rows, int32_t *level, const int32_t *__restrict__ in_ptr,
                                                       const int32_t *__restrict__ in_col, const uint32_t *__restrict__ bm,
                                                       uint32_t *bm_next, const WlPiece *__restrict__ rpieces, int32_t n_rpieces,
                                                       WlPart *__restrict__ part) {
  if (ctl->step != L || ctl->mode != 1) return;
  const int lane = wl_lane();
  uint32_t found = 0, looked = 0;
  // 64 consecutive rows per wave step: level and in_ptr are read coalesced
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const int64_t r = base + lane;
    const bool open = r < rows && level[r] == -1;
    const int32_t s = open ? in_ptr[r] : 0;
    const int32_t len = open ? in_ptr[r + 1] - s : 0;
    bool hit = false;
    if (len <= BFS_BU_SHORT)
      for (int32_t j = 0; j < len; j++) {
        looked++;
        if (bfs_bit(bm, in_col[s + j])) { hit = true; break; }   // the early exit
      }
    uint64_t m = __ballot(len > BFS_BU_SHORT && len <= BFS_ROW_PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      uint32_t seen = 0;
      const bool h = bfs_wave_search(in_col, bm, sb, sb + lb, lane, &seen);
      if (lane == src) { hit = h; looked += seen; }
    }
    if (hit) level[r] = L + 1;   // (only this lane writes row r: longer rows go through the pieces below)
    const uint64_t hm = __ballot(hit);
    // (atomic: a long row of the same word may set its bit from another wave)
    if (lane == 0 && (uint32_t)hm) bfs_or(&bm_next[base >> 5], (uint32_t)hm);
    if (lane == 32 && (uint32_t)(hm >> 32)) bfs_or(&bm_next[(base >> 5) + 1], (uint32_t)(hm >> 32));
    found += hit ? 1u : 0u;
  }
  // Rows above BFS_ROW_PIECE: one wave per piece.  A piece that comes late may find the row already claimed by another
  // piece and skips it; two pieces that both find a frontier column race for the row with a compare-and-swap -- both
  // would write the same level, but only one may count the row.
  for (int64_t i = wl_wave(); i < n_rpieces; i += wl_waves()) {
    const WlPiece pc = rpieces[i];
    const int32_t r = (int32_t)pc.id;
    if (level[r] != -1) continue;
    const int32_t s = in_ptr[r] + (int32_t)pc.off;
    const int32_t e = min(s + BFS_ROW_PIECE, in_ptr[r + 1]);
    uint32_t seen = 0;
    const bool h = bfs_wave_search(in_col, bm, s, e, lane, &seen);
    if (lane == 0) {
      looked += seen;
      int32_t expect = -1;
      if (h && __hip_atomic_compare_exchange_strong(&level[r], &expect, L + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT)) {
        bfs_or(&bm_next[r >> 5], 1u << (r & 31));
        found++;
      }
    }
  }
  wl_block_part(part, found, looked);
}

// The frontier a bottom-up step left as a bitmap -> queue (and the pieces of its long out-lists), for a top-down step.
__global__ __launch_bounds__(WL_BS) void bfs_queue_from_bitmap(BfsCtl *ctl, int L, int32_t words, const uint32_t *__restrict__ bm,
                                                                const int32_t *__restrict__ out_ptr, uint32_t *__restrict__ queue,
                                                                WlPiece *__restrict__ pl) {
  if (ctl->step != L || ctl->mode != 0 || ctl->have_queue != 0) return;
  const int lane = wl_lane(), p = L & 1;
  for (int64_t base = wl_wave() * 64; base < words; base += wl_waves() * 64) {
    uint32_t w = base + lane < words ? bm[base + lane] : 0u;
    const uint32_t cnt = (uint32_t)__popc(w);
    uint32_t incl = cnt;   // inclusive prefix sum over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
      if (lane >= o) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    if (total == 0) continue;
    uint32_t first = 0;
    if (lane == 63) first = wl_add(&ctl->qcount[p], total);   // one add per 2048 vertices
    uint32_t at = (uint32_t)__shfl((int)first, 63) + incl - cnt;
    while (w) {
      const int32_t v = (int32_t)((base + lane) * 32 + (__ffs((int)w) - 1));
      w &= w - 1;
      queue[at++] = (uint32_t)v;
      wl_push_pieces<BFS_OUT_PIECE>(&ctl->qpieces[p], (uint32_t)v, (uint32_t)(out_ptr[v + 1] - out_ptr[v]), pl);
    }
  }
}

// Closes step L (slot k of the batch); L = -1 closes bfs_init and chooses the direction of step 0.  Every workgroup
// clears its share of the bitmap the step consumed, whether the step ran or not (after the end of the search nobody
// reads a bitmap); workgroup 0 sums the WlParts and its first lane applies the rule:
//   after a top-down step (and for step 0): bottom-up iff m > up_edges (= up_share * edges);
//   after a bottom-up step: top-down iff |F| < down_rows (= down_share * rows).
__global__ __launch_bounds__(WL_BS) void bfs_decide(BfsCtl *ctl, int k, int L, int nparts, const WlPart *__restrict__ part,
                                                     uint32_t *__restrict__ bm, int32_t words, double up_edges, double down_rows) {
  if (L >= 0)
    for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < words; i += (int64_t)gridDim.x * WL_BS) bm[i] = 0u;
  if (blockIdx.x != 0) return;
  if (!wl_from_thread0(L < 0 || ctl->step == L)) return;
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t a = sums.a, b = sums.b;
  if (L < 0) {
    const uint32_t nsrc = ctl->qcount[0];
    ctl->nsrc = nsrc; ctl->fsize = nsrc;
    ctl->finished = nsrc == 0 ? 1 : 0;
    ctl->step = nsrc == 0 ? -1 : 0;
    ctl->mode = (double)a > up_edges ? 1 : 0;
    ctl->have_queue = 1;
    return;
  }
  const int p = L & 1, mode = ctl->mode;   // (this thread alone stores it, below)
  const uint32_t found = mode == 0 ? ctl->qcount[p ^ 1] : a;
  const uint32_t edges = mode == 0 ? a : b;
  const int done = found == 0 ? 1 : 0;
  ctl->rec[k] = BfsRec{1, mode, done, found, edges};
  ctl->qcount[p] = 0; ctl->qpieces[p] = 0;
  if (done) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->mode = mode == 0 ? ((double)b > up_edges ? 1 : 0) : ((double)found < down_rows ? 0 : 1);
  ctl->have_queue = mode == 0 ? 1 : 0;
  ctl->fsize = found;
  ctl->step = L + 1;
}

// parent[r] = the smallest c with an edge c -> r and level[c] == level[r] - 1 (wl_rows_min: the host fills parent with
// -1 first).
__global__ __launch_bounds__(WL_BS) void bfs_parents(int32_t rows, const int32_t *__restrict__ level, const int32_t *__restrict__ in_ptr,
                                                     const int32_t *__restrict__ in_col, const WlPiece *__restrict__ rpieces,
                                                     int32_t n_rpieces, int32_t *parent) {
  wl_rows_min<BFS_SHORT, BFS_ROW_PIECE>(
      rows, in_ptr, in_col, rpieces, n_rpieces, parent,
      [&](int32_t r, uint32_t *want) { const int32_t lv = level[r]; *want = (uint32_t)(lv - 1); return lv > 0; },
      [&](int32_t j, uint32_t want) { return level[in_col[j]] == (int32_t)want; });
}

} // namespace sh
