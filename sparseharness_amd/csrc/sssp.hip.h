// sssp.hip.h -- kernels of sh_sssp: a bucketed, push-based label-correcting single-source shortest path search
// (near-far: Davidson, Baxter, Garland, Owens: "Work-efficient parallel GPU methods for single-source shortest paths",
// IPDPS 2014; delta-stepping: Meyer, Sanders, 2003) that reports the distance of every vertex and, on request, a
// canonical predecessor (DESIGN.md "6f Bucketed SSSP").
//
// The graph lives in a layout of its own (sh_sssp_graph): the out-edges by source vertex (out_ptr / out_row / out_w,
// w = |a| as float) and the in-edges by row (in_ptr / in_col / in_w, stored order of the survivors kept) for the
// predecessor pass.  dist holds the bits of non-negative floats that are not NaN, so their order is that of their bits
// as unsigned words (as frontier.hip.h relies on for (min,+) partials) and a relaxation is one UNSIGNED atomic min.
//
// Lists.  NEAR list R & 1 holds the vertices round R relaxes from; relaxations of round R file into the other near list
// (new value below the threshold) or into the live FAR list (otherwise).  When a round leaves the next near list empty
// the following round opens with a split: the threshold jumps to the end of the bucket [k * delta, (k + 1) * delta) that
// holds the smallest live far distance (empty buckets cost nothing), the live far entries below it move to the near
// list and the others to the second far list.
//
// Invariant 1: NO LIST CAN OVERFLOW ON ANY INPUT.  stamp[v] is 0 (never filed), 1 (filed far) or R + 2 (filed into the
// near list of round R); it only grows (atomic max) and whoever raises it files v:
//   - into a near list at most once per round: only the lane that sees a stamp below the round's tag appends;
//   - into the far list at most once per call: only the lane that sees 0 appends.  A vertex that ever was near has
//     dist < threshold for good (dist only falls, the threshold only rises), so it never needs the far list again.
// A far entry is live while stamp[v] == 1; one whose vertex moved to a near list meanwhile is stale and is dropped by
// the split.  A near entry is always read with the dist of the moment, so an entry that came late costs one walk of an
// out-list that improves nothing.  Lists of `rows` entries therefore suffice, and the piece lists are bounded by
// edges / 1024 + 1 as in bfs.hip.h.
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE.  There is no spin loop and no handshake between
// workgroups inside a launch; every loop is bounded by a length read once at its start; the gate words a kernel reads
// were written by a launch that ended before it.  max_rounds bounds the call.
//
// A round is four launches (sssp_split phase 0 and phase 1, sssp_relax, sssp_decide); each returns at once unless
// SsspCtl says that this round runs (and, for the two split launches, opens with a split).  sssp_preds is one
// row-parallel pass after the search, so the search carries no predecessor atomics.
#pragma once
#include "bfs.hip.h"

namespace sh {

constexpr int SSSP_BS = 256;
constexpr int SSSP_SHORT = 8;            // out-lists / rows up to this many edges: one lane each
constexpr int SSSP_OUT_PIECE = BFS_OUT_PIECE;   // out-lists above this are relaxed in pieces (bfs_push_pieces cuts them)
constexpr int SSSP_ROW_PIECE = BFS_ROW_PIECE;   // rows above this are searched in pieces (bfs_row_pieces cuts them)
constexpr int SSSP_BATCH = 32;           // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int SSSP_MAX_BLOCKS = 1024;    // workgroups of a launch at most: one BfsPart and one minimum each
constexpr int SSSP_CTL_BYTES = 2048;     // device bytes set aside for SsspCtl
constexpr int SSSP_PART_BYTES = 16 * SSSP_MAX_BLOCKS;
constexpr int SSSP_PMIN_BYTES = 4 * SSSP_MAX_BLOCKS;
constexpr uint32_t SSSP_FLT_MAX = 0x7F7FFFFFu, SSSP_INF = 0x7F800000u, SSSP_FAR = 1u;

struct SsspRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran, split;
  uint32_t size, edges;
};
struct SsspCtl {
  uint32_t ncount[2], npieces[2];   // length of near list 0 / 1 and of its list of long out-list pieces
  uint32_t fcount[2];               // length of far list 0 / 1
  int32_t round;                    // the round that runs next (-1 once the search has finished)
  int32_t need_split;               // it opens with a split
  int32_t fsel;                     // the live far list
  int32_t finished;
  uint32_t thr, thr_new;            // the threshold (bits of the smallest float >= it); what the split of this round chose
  uint32_t nsrc, buckets;
  uint64_t relaxed, reached;        // edges looked at / vertices with dist < FLT_MAX so far
  SsspRec rec[SSSP_BATCH];
};

#define SSSP_LANE ((int)(threadIdx.x & 63))
#define SSSP_WAVE ((int64_t)blockIdx.x * (SSSP_BS / 64) + (threadIdx.x >> 6))
#define SSSP_WAVES ((int64_t)gridDim.x * (SSSP_BS / 64))

__device__ __forceinline__ uint32_t sssp_umin(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t sssp_umax(uint32_t *p, uint32_t v) {
  return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// d0 = min(|x0|, FLT_MAX): what the first launch of sh_iterate makes of an infinite start
__device__ __forceinline__ uint32_t sssp_start_bits(uint32_t x) { return min(x & 0x7FFFFFFFu, SSSP_FLT_MAX); }

// ---- building the handle (once)
// flag[j] = entry j is an edge: column inside the matrix, |a| finite (flag[nnz] = 0 closes the scan)
__global__ __launch_bounds__(SSSP_BS) void sssp_edge_flag(const int32_t *__restrict__ col_idx, const uint32_t *__restrict__ val,
                                                          int64_t nnz, int32_t cols, uint32_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * SSSP_BS + threadIdx.x;
  if (j < nnz) flag[j] = ((val[j] & 0x7FFFFFFFu) < SSSP_INF && (uint32_t)col_idx[j] < (uint32_t)cols) ? 1u : 0u;
  else if (j == nnz) flag[j] = 0u;
}
// pos = exclusive scan of flag: edge j goes to in_col / in_w[pos[j]], its weight as |a|
__global__ __launch_bounds__(SSSP_BS) void sssp_edge_compact(const int32_t *__restrict__ col_idx, const uint32_t *__restrict__ val,
                                                             const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                             int64_t nnz, int32_t *__restrict__ in_col, uint32_t *__restrict__ in_w) {
  const int64_t j = (int64_t)blockIdx.x * SSSP_BS + threadIdx.x;
  if (j < nnz && flag[j]) {
    in_col[pos[j]] = col_idx[j];
    in_w[pos[j]] = val[j] & 0x7FFFFFFFu;
  }
}
// frontier_scatter carrying the weight (every column is inside the matrix here: the edges are compacted already)
__global__ __launch_bounds__(SSSP_BS) void sssp_scatter(const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_col,
                                                        const uint32_t *__restrict__ in_w, int64_t edges, int32_t rows,
                                                        uint32_t *__restrict__ cursor, int32_t *__restrict__ out_row,
                                                        uint32_t *__restrict__ out_w) {
  const int64_t j = (int64_t)blockIdx.x * SSSP_BS + threadIdx.x;
  if (j >= edges) return;
  const int32_t c = in_col[j];
  int32_t lo = 0, hi = rows;   // last r with in_ptr[r] <= j
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if ((int64_t)in_ptr[mid] <= j) lo = mid; else hi = mid;
  }
  const uint32_t at = fr_add(&cursor[c], 1u);
  out_row[at] = lo;
  out_w[at] = in_w[j];
}
// sum[b] = the sum of the weights workgroup b strides over, in double (the host adds the partials: the default delta)
__global__ __launch_bounds__(SSSP_BS) void sssp_weight_sum(const uint32_t *__restrict__ w, int64_t edges, double *__restrict__ sum) {
  __shared__ double s_sum[SSSP_BS];
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * SSSP_BS + threadIdx.x; j < edges; j += (int64_t)gridDim.x * SSSP_BS)
    acc += (double)__uint_as_float(w[j]);
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int o = SSSP_BS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sum[blockIdx.x] = s_sum[0];
}

// ---- the search
// dist = d0, every stamp written; the sources (d0 < FLT_MAX) into far list 0, from which the split of round 0 takes
// the first bucket -- one source at 0, several sources and sources with offsets alike.
__global__ __launch_bounds__(SSSP_BS) void sssp_init(SsspCtl *ctl, int32_t rows, const uint32_t *__restrict__ x0,
                                                     uint32_t *__restrict__ dist, uint32_t *__restrict__ stamp,
                                                     uint32_t *__restrict__ far) {
  const int lane = SSSP_LANE;
  for (int64_t base = SSSP_WAVE * 64; base < rows; base += SSSP_WAVES * 64) {
    const int64_t r = base + lane;
    const uint32_t d = r < rows ? sssp_start_bits(x0[r]) : SSSP_FLT_MAX;
    const bool src = d < SSSP_FLT_MAX;
    if (r < rows) { dist[r] = d; stamp[r] = src ? SSSP_FAR : 0u; }
    const uint32_t at = fr_wave_append(&ctl->fcount[0], src, lane);
    if (src) far[at] = (uint32_t)r;
  }
}

// Phase 0 of sssp_split: the smallest live far distance, per workgroup (0xFFFFFFFF: none).
__device__ __forceinline__ void sssp_split_min(const SsspCtl *ctl, const uint32_t *__restrict__ dist,
                                               const uint32_t *__restrict__ stamp, const uint32_t *__restrict__ far0,
                                               const uint32_t *__restrict__ far1, uint32_t *__restrict__ pmin) {
  const uint32_t *__restrict__ far = ctl->fsel ? far1 : far0;
  const int64_t n = ctl->fcount[ctl->fsel];
  uint32_t m = 0xFFFFFFFFu;
  for (int64_t i = (int64_t)blockIdx.x * SSSP_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SSSP_BS) {
    const uint32_t v = far[i];
    if (stamp[v] == SSSP_FAR) m = min(m, dist[v]);
  }
  for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
  __shared__ uint32_t s_m[SSSP_BS / 64];
  if (SSSP_LANE == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SSSP_BS / 64; w++) m = min(m, s_m[w]);
    pmin[blockIdx.x] = m;
  }
}

// The end of the bucket that holds distance m, as the bits of the smallest float that is not below it.  It is above m
// whatever delta is (should the product round down to m, or delta vanish beside m, the search degrades towards one
// bucket; the result does not depend on the threshold).
__device__ __forceinline__ uint32_t sssp_bucket_end(uint32_t m_bits, double delta) {
  const double m = (double)__uint_as_float(m_bits);
  double t = (floor(m / delta) + 1.0) * delta;   // (delta = +Inf: m / Inf = 0, 1 * Inf = Inf, one bucket)
  if (!(t > m)) t = m + delta;
  if (!(t > m)) return SSSP_INF;
  return t > 3.4028234663852886e38 ? SSSP_INF : __float_as_uint(__double2float_ru(t));
}

// Phase 1 of sssp_split (a launch of its own, after phase 0 has ended): every workgroup reduces the minima of phase 0
// by itself (at most 1024 words out of L2) and so knows the new threshold without waiting for anybody; then the live far
// entries below it go to the near list of round R (with their out-list pieces), the other live ones to the second far
// list, the stale ones nowhere.
__device__ __forceinline__ void sssp_split_move(SsspCtl *ctl, int R, int nparts, double delta, const uint32_t *__restrict__ pmin,
                                                const uint32_t *__restrict__ dist, uint32_t *__restrict__ stamp,
                                                const int32_t *__restrict__ out_ptr, uint32_t *__restrict__ far0,
                                                uint32_t *__restrict__ far1, uint32_t *__restrict__ near,
                                                FrPiece *__restrict__ pl) {
  __shared__ uint32_t s_m[SSSP_BS / 64];
  uint32_t m = 0xFFFFFFFFu;
  for (int i = (int)threadIdx.x; i < nparts; i += SSSP_BS) m = min(m, pmin[i]);
  for (int o = 32; o > 0; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
  if (SSSP_LANE == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  m = s_m[0];
  for (int w = 1; w < SSSP_BS / 64; w++) m = min(m, s_m[w]);
  const uint32_t thr = m == 0xFFFFFFFFu ? ctl->thr : sssp_bucket_end(m, delta);
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->thr_new = thr;   // (read by sssp_relax and sssp_decide, not in this launch)
  const int f = ctl->fsel, p = R & 1, lane = SSSP_LANE;
  const uint32_t *__restrict__ far = f ? far1 : far0;
  uint32_t *__restrict__ keep = f ? far0 : far1;
  const int64_t n = ctl->fcount[f];
  const uint32_t tag = (uint32_t)R + 2u;
  for (int64_t base = SSSP_WAVE * 64; base < n; base += SSSP_WAVES * 64) {
    const bool valid = base + lane < n;
    const uint32_t v = valid ? far[base + lane] : 0u;
    const bool live = valid && stamp[v] == SSSP_FAR;
    const bool now = live && dist[v] < thr;
    const uint32_t at = fr_wave_append(&ctl->ncount[p], now, lane);
    if (now) {
      stamp[v] = tag;   // (no relaxation runs beside a split: a plain store)
      near[at] = v;
      bfs_push_pieces(&ctl->npieces[p], (int32_t)v, (uint32_t)(out_ptr[v + 1] - out_ptr[v]), pl);
    }
    const uint32_t kat = fr_wave_append(&ctl->fcount[f ^ 1], live && !now, lane);
    if (live && !now) keep[kat] = v;
  }
}

// When the near list ran empty: move the threshold and carry over what falls below it.  Two launches per round (phase
// 0, phase 1); both return at once unless round R opens with a split.
__global__ __launch_bounds__(SSSP_BS) void sssp_split(SsspCtl *ctl, int R, int phase, int nparts, double delta, uint32_t *__restrict__ pmin,
                                                      const uint32_t *__restrict__ dist, uint32_t *__restrict__ stamp,
                                                      const int32_t *__restrict__ out_ptr, uint32_t *__restrict__ far0,
                                                      uint32_t *__restrict__ far1, uint32_t *__restrict__ near,
                                                      FrPiece *__restrict__ pl) {
  if (ctl->round != R || ctl->need_split == 0) return;
  if (phase == 0) sssp_split_min(ctl, dist, stamp, far0, far1, pmin);
  else sssp_split_move(ctl, R, nparts, delta, pmin, dist, stamp, out_ptr, far0, far1, near, pl);
}

// dist[r] = min(dist[r], nd); the lane that lowered the word files r (see invariant 1).  -> 1 when r was reached for
// the first time (exactly one lane sees FLT_MAX come back).
__device__ __forceinline__ uint32_t sssp_try(SsspCtl *ctl, int q, int f, int32_t r, uint32_t nd, uint32_t thr, uint32_t tag,
                                             uint32_t *dist, uint32_t *stamp, const int32_t *__restrict__ out_ptr,
                                             uint32_t *__restrict__ near_next, FrPiece *__restrict__ pl_next,
                                             uint32_t *__restrict__ far) {
  if (nd >= dist[r]) return 0;   // (a stale word is a larger one: dist only falls, so this never skips an improvement)
  const uint32_t old = sssp_umin(&dist[r], nd);
  if (old <= nd) return 0;
  if (nd < thr) {
    if (sssp_umax(&stamp[r], tag) < tag) {
      near_next[bfs_append_here(&ctl->ncount[q])] = (uint32_t)r;
      bfs_push_pieces(&ctl->npieces[q], r, (uint32_t)(out_ptr[r + 1] - out_ptr[r]), pl_next);
    }
  } else if (sssp_umax(&stamp[r], SSSP_FAR) == 0u) {
    far[bfs_append_here(&ctl->fcount[f])] = (uint32_t)r;
  }
  return old == SSSP_FLT_MAX ? 1u : 0u;
}

// Round R: every vertex of near list R & 1 offers fl32(dist[v] + w) to the heads of its out-edges.
__global__ __launch_bounds__(SSSP_BS) void sssp_relax(SsspCtl *ctl, int R, uint32_t *dist, uint32_t *stamp,
                                                      const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ out_row,
                                                      const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ near,
                                                      const FrPiece *__restrict__ pl, uint32_t *__restrict__ near_next,
                                                      FrPiece *__restrict__ pl_next, uint32_t *__restrict__ far0,
                                                      uint32_t *__restrict__ far1, BfsPart *__restrict__ part) {
  if (ctl->round != R) return;
  const int lane = SSSP_LANE, p = R & 1, q = p ^ 1;
  const int split = ctl->need_split;
  const int f = split ? ctl->fsel ^ 1 : ctl->fsel;   // (a split of this round has moved the live far list)
  const uint32_t thr = split ? ctl->thr_new : ctl->thr;
  uint32_t *__restrict__ far = f ? far1 : far0;
  const uint32_t tag = (uint32_t)R + 3u;             // the near list of round R + 1
  const int64_t n = ctl->ncount[p], np = ctl->npieces[p];
  uint32_t looked = 0, newly = 0;
#define SSSP_TRY(j, d)                                                                                                        \
  newly += sssp_try(ctl, q, f, out_row[j], __float_as_uint(__uint_as_float(d) + __uint_as_float(out_w[j])), thr, tag, dist, \
                    stamp, out_ptr, near_next, pl_next, far)
  for (int64_t base = SSSP_WAVE * 64; base < n; base += SSSP_WAVES * 64) {
    const bool valid = base + lane < n;
    const int32_t v = valid ? (int32_t)near[base + lane] : 0;
    const int32_t s = valid ? out_ptr[v] : 0;
    const int32_t len = valid ? out_ptr[v + 1] - s : 0;
    const uint32_t d = valid ? dist[v] : SSSP_FLT_MAX;
    looked += (uint32_t)len;
    if (len <= SSSP_SHORT)
      for (int32_t j = 0; j < len; j++) SSSP_TRY(s + j, d);
    uint64_t m = __ballot(len > SSSP_SHORT && len <= SSSP_OUT_PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const uint32_t db = (uint32_t)__shfl((int)d, src);
      for (int32_t j = lane; j < lb; j += 64) SSSP_TRY(sb + j, db);
    }
  }
  for (int64_t i = SSSP_WAVE; i < np; i += SSSP_WAVES) {   // a hub's out-list: one wave per piece
    const FrPiece pc = pl[i];
    const int32_t s = out_ptr[pc.id] + (int32_t)pc.off;
    const int32_t e = min(s + SSSP_OUT_PIECE, out_ptr[pc.id + 1]);
    const uint32_t d = dist[pc.id];
    for (int32_t j = s + lane; j < e; j += 64) SSSP_TRY(j, d);
  }
#undef SSSP_TRY
  bfs_block_part(part, looked, newly);
}

// Closes round R (slot k of the batch); R = -1 closes sssp_init.  One workgroup sums the BfsParts (no atomics on one
// word: they retire about 6 ns apart, see frontier_detect) and its first lane turns the page.
__global__ __launch_bounds__(SSSP_BS) void sssp_decide(SsspCtl *ctl, int k, int R, int nparts, const BfsPart *__restrict__ part) {
  __shared__ uint32_t s_a[SSSP_BS], s_b[SSSP_BS];
  __shared__ int32_t s_go;
  if (threadIdx.x == 0) s_go = (R < 0 || ctl->round == R) ? 1 : 0;
  __syncthreads();
  if (!s_go) return;
  if (R < 0) {
    if (threadIdx.x != 0) return;
    const uint32_t nsrc = ctl->fcount[0];
    ctl->nsrc = nsrc; ctl->reached = nsrc; ctl->relaxed = 0; ctl->buckets = 0;
    ctl->thr = 0u; ctl->thr_new = 0u; ctl->fsel = 0;
    ctl->finished = nsrc == 0 ? 1 : 0;
    ctl->round = nsrc == 0 ? -1 : 0;
    ctl->need_split = nsrc == 0 ? 0 : 1;
    return;
  }
  uint32_t a = 0, b = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += SSSP_BS) { a += part[i].a; b += part[i].b; }
  s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0; b = 0;
  for (int i = 0; i < SSSP_BS; i++) { a += s_a[i]; b += s_b[i]; }
  const int p = R & 1, split = ctl->need_split;
  if (split) {   // the far list the split consumed is empty now; its survivors and this round's arrivals are in the other
    ctl->fcount[ctl->fsel] = 0;
    ctl->fsel ^= 1;
    if (ctl->thr_new != ctl->thr) ctl->buckets++;
    ctl->thr = ctl->thr_new;
  }
  ctl->rec[k] = SsspRec{1, split, ctl->ncount[p], a};
  ctl->relaxed += a;
  ctl->reached += b;
  ctl->ncount[p] = 0; ctl->npieces[p] = 0;
  if (ctl->ncount[p ^ 1] > 0) { ctl->need_split = 0; ctl->round = R + 1; }
  else if (ctl->fcount[ctl->fsel] > 0) { ctl->need_split = 1; ctl->round = R + 1; }
  else { ctl->need_split = 0; ctl->finished = 1; ctl->round = -1; }
}

// pred[r] = the smallest c with an edge c -> r and bits(fl32(dist[c] + w)) == bits(dist[r]), for the rows whose word is
// not their start value any more.  The host fills pred with -1 first; pieces of long rows meet in pred[r] by an UNSIGNED
// atomic min, under which -1 (no candidate yet) is the largest word.
__global__ __launch_bounds__(SSSP_BS) void sssp_preds(int32_t rows, const uint32_t *__restrict__ x0, const uint32_t *__restrict__ dist,
                                                      const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_col,
                                                      const uint32_t *__restrict__ in_w, const FrPiece *__restrict__ rpieces,
                                                      int32_t n_rpieces, int32_t *pred) {
  const int lane = SSSP_LANE;
#define SSSP_HIT(j, want) (__float_as_uint(__uint_as_float(dist[in_col[j]]) + __uint_as_float(in_w[j])) == (want))
  for (int64_t base = SSSP_WAVE * 64; base < rows; base += SSSP_WAVES * 64) {
    const int64_t r = base + lane;
    const uint32_t dr = r < rows ? dist[r] : 0u;
    const bool moved = r < rows && dr != sssp_start_bits(x0[r]);
    const int32_t s = moved ? in_ptr[r] : 0;
    const int32_t len = moved ? in_ptr[r + 1] - s : 0;
    uint32_t best = 0xFFFFFFFFu;
    if (len <= SSSP_SHORT)
      for (int32_t j = s; j < s + len; j++)
        if (SSSP_HIT(j, dr)) best = min(best, (uint32_t)in_col[j]);
    uint64_t m = __ballot(len > SSSP_SHORT && len <= SSSP_ROW_PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const uint32_t want = (uint32_t)__shfl((int)dr, src);
      uint32_t mine = 0xFFFFFFFFu;
      for (int32_t j = sb + lane; j < sb + lb; j += 64)
        if (SSSP_HIT(j, want)) mine = min(mine, (uint32_t)in_col[j]);
      for (int o = 32; o > 0; o >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, o));
      if (lane == src) best = mine;
    }
    if (len > 0 && len <= SSSP_ROW_PIECE) pred[r] = (int32_t)best;
  }
  for (int64_t i = SSSP_WAVE; i < n_rpieces; i += SSSP_WAVES) {
    const FrPiece pc = rpieces[i];
    const int32_t r = (int32_t)pc.id;
    const uint32_t want = dist[r];
    if (want == sssp_start_bits(x0[r])) continue;
    const int32_t s = in_ptr[r] + (int32_t)pc.off;
    const int32_t e = min(s + SSSP_ROW_PIECE, in_ptr[r + 1]);
    uint32_t mine = 0xFFFFFFFFu;
    for (int32_t j = s + lane; j < e; j += 64)
      if (SSSP_HIT(j, want)) mine = min(mine, (uint32_t)in_col[j]);
    for (int o = 32; o > 0; o >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, o));
    if (lane == 0 && mine != 0xFFFFFFFFu) (void)sssp_umin((uint32_t *)&pred[r], mine);
  }
#undef SSSP_HIT
}

#undef SSSP_LANE
#undef SSSP_WAVE
#undef SSSP_WAVES

} // namespace sh
