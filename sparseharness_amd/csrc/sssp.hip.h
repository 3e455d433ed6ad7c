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
// edges / 1024 + 1 (wl_push_pieces).
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE.  There is no spin loop and no handshake between
// workgroups inside a launch; every loop is bounded by a length read once at its start; the gate words a kernel reads
// were written by a launch that ended before it.  max_rounds bounds the call.
//
// A round is four launches (sssp_split phase 0 and phase 1, sssp_relax, sssp_decide); each returns at once unless
// SsspCtl says that this round runs (and, for the two split launches, opens with a split).  sssp_preds is one
// row-parallel pass after the search, so the search carries no predecessor atomics.
//
// Work distribution as worklist.hip.h describes it.  The handle is built by its kernels (wl_edge_flag<SsspKeep>,
// wl_edge_compact, wl_row_starts, wl_row_pieces<SSSP_ROW_PIECE>, wl_col_hist, wl_transpose_scatter, the last two and
// the compaction carrying the weights) and by sssp_weight_sum.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int SSSP_SHORT = 8;            // out-lists / rows up to this many edges: one lane each
constexpr int SSSP_OUT_PIECE = 2048;     // out-lists above this are relaxed in pieces of this many edges
constexpr int SSSP_ROW_PIECE = 4096;     // rows above this are searched in pieces of this many edges (a static list)
constexpr int SSSP_BATCH = 32;           // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int SSSP_MAX_BLOCKS = 1024;    // workgroups of a launch at most: one WlPart and one minimum each
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

// d0 = min(|x0|, FLT_MAX): what the first launch of sh_iterate makes of an infinite start
__device__ __forceinline__ uint32_t sssp_start_bits(uint32_t x) { return min(x & 0x7FFFFFFFu, SSSP_FLT_MAX); }

struct SsspKeep {   // wl_edge_flag: an entry is an edge when |a| is finite (and its column is inside the matrix)
  __device__ static bool value(uint32_t v) { return (v & 0x7FFFFFFFu) < SSSP_INF; }
};

// ---- building the handle (once): what worklist.hip.h does not have
// sum[b] = the sum of the weights workgroup b strides over, in double (the host adds the partials: the default delta).
// Not wl_block_fold, and its tree is not to be touched: doubles added in another order differ in their last bits, and
// with them the default delta and the round counts that depend on it.
__global__ __launch_bounds__(WL_BS) void sssp_weight_sum(const uint32_t *__restrict__ w, int64_t edges, double *__restrict__ sum) {
  __shared__ double s_sum[WL_BS];
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x; j < edges; j += (int64_t)gridDim.x * WL_BS)
    acc += (double)__uint_as_float(w[j]);
  s_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int o = WL_BS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sum[blockIdx.x] = s_sum[0];
}

// ---- the search
// dist = d0, every stamp written; the sources (d0 < FLT_MAX) into far list 0, from which the split of round 0 takes
// the first bucket -- one source at 0, several sources and sources with offsets alike.
__global__ __launch_bounds__(WL_BS) void sssp_init(SsspCtl *ctl, int32_t rows, const uint32_t *__restrict__ x0,
                                                     uint32_t *__restrict__ dist, uint32_t *__restrict__ stamp,
                                                     uint32_t *__restrict__ far) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const int64_t r = base + lane;
    const uint32_t d = r < rows ? sssp_start_bits(x0[r]) : SSSP_FLT_MAX;
    const bool src = d < SSSP_FLT_MAX;
    if (r < rows) { dist[r] = d; stamp[r] = src ? SSSP_FAR : 0u; }
    const uint32_t at = wl_wave_append(&ctl->fcount[0], src, lane);
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
  for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WL_BS) {
    const uint32_t v = far[i];
    if (stamp[v] == SSSP_FAR) m = min(m, dist[v]);
  }
  m = wl_block_fold<WlMin>(m);
  if (threadIdx.x == 0) pmin[blockIdx.x] = m;
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
                                                WlPiece *__restrict__ pl) {
  uint32_t m = 0xFFFFFFFFu;
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) m = min(m, pmin[i]);
  m = wl_block_fold<WlMin>(m);
  const uint32_t thr = m == 0xFFFFFFFFu ? ctl->thr : sssp_bucket_end(m, delta);
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->thr_new = thr;   // (read by sssp_relax and sssp_decide, not in this launch)
  const int f = ctl->fsel, p = R & 1, lane = wl_lane();
  const uint32_t *__restrict__ far = f ? far1 : far0;
  uint32_t *__restrict__ keep = f ? far0 : far1;
  const int64_t n = ctl->fcount[f];
  const uint32_t tag = (uint32_t)R + 2u;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const uint32_t v = valid ? far[base + lane] : 0u;
    const bool live = valid && stamp[v] == SSSP_FAR;
    const bool now = live && dist[v] < thr;
    const uint32_t at = wl_wave_append(&ctl->ncount[p], now, lane);
    if (now) {
      stamp[v] = tag;   // (no relaxation runs beside a split: a plain store)
      near[at] = v;
      wl_push_pieces<SSSP_OUT_PIECE>(&ctl->npieces[p], v, (uint32_t)(out_ptr[v + 1] - out_ptr[v]), pl);
    }
    const uint32_t kat = wl_wave_append(&ctl->fcount[f ^ 1], live && !now, lane);
    if (live && !now) keep[kat] = v;
  }
}

// When the near list ran empty: move the threshold and carry over what falls below it.  Two launches per round (phase
// 0, phase 1); both return at once unless round R opens with a split.
__global__ __launch_bounds__(WL_BS) void sssp_split(SsspCtl *ctl, int R, int phase, int nparts, double delta, uint32_t *__restrict__ pmin,
                                                      const uint32_t *__restrict__ dist, uint32_t *__restrict__ stamp,
                                                      const int32_t *__restrict__ out_ptr, uint32_t *__restrict__ far0,
                                                      uint32_t *__restrict__ far1, uint32_t *__restrict__ near,
                                                      WlPiece *__restrict__ pl) {
  if (ctl->round != R || ctl->need_split == 0) return;
  if (phase == 0) sssp_split_min(ctl, dist, stamp, far0, far1, pmin);
  else sssp_split_move(ctl, R, nparts, delta, pmin, dist, stamp, out_ptr, far0, far1, near, pl);
}

// dist[r] = min(dist[r], nd); the lane that lowered the word files r (see invariant 1).  -> 1 when r was reached for
// the first time (exactly one lane sees FLT_MAX come back).
__device__ __forceinline__ uint32_t sssp_try(SsspCtl *ctl, int q, int f, int32_t r, uint32_t nd, uint32_t thr, uint32_t tag,
                                             uint32_t *dist, uint32_t *stamp, const int32_t *__restrict__ out_ptr,
                                             uint32_t *__restrict__ near_next, WlPiece *__restrict__ pl_next,
                                             uint32_t *__restrict__ far) {
  if (nd >= dist[r]) return 0;   // (a stale word is a larger one: dist only falls, so this never skips an improvement)
  const uint32_t old = wl_umin(&dist[r], nd);
  if (old <= nd) return 0;
  if (nd < thr) {
    if (wl_umax(&stamp[r], tag) < tag) {
      near_next[wl_append_here(&ctl->ncount[q])] = (uint32_t)r;
      wl_push_pieces<SSSP_OUT_PIECE>(&ctl->npieces[q], (uint32_t)r, (uint32_t)(out_ptr[r + 1] - out_ptr[r]), pl_next);
    }
  } else if (wl_umax(&stamp[r], SSSP_FAR) == 0u) {
    far[wl_append_here(&ctl->fcount[f])] = (uint32_t)r;
  }
  return old == SSSP_FLT_MAX ? 1u : 0u;
}

// Round R: every vertex of near list R & 1 offers fl32(dist[v] + w) to the heads of its out-edges.
__global__ __launch_bounds__(WL_BS) void sssp_relax(SsspCtl *ctl, int R, uint32_t *dist, uint32_t *stamp,
                                                      const int32_t *__restrict__ out_ptr, const int32_t *__restrict__ out_row,
                                                      const uint32_t *__restrict__ out_w, const uint32_t *__restrict__ near,
                                                      const WlPiece *__restrict__ pl, uint32_t *__restrict__ near_next,
                                                      WlPiece *__restrict__ pl_next, uint32_t *__restrict__ far0,
                                                      uint32_t *__restrict__ far1, WlPart *__restrict__ part) {
  if (ctl->round != R) return;
  const int p = R & 1, q = p ^ 1;
  const int split = ctl->need_split;
  const int f = split ? ctl->fsel ^ 1 : ctl->fsel;   // (a split of this round has moved the live far list)
  const uint32_t thr = split ? ctl->thr_new : ctl->thr;
  uint32_t *__restrict__ far = f ? far1 : far0;
  const uint32_t tag = (uint32_t)R + 3u;             // the near list of round R + 1
  uint32_t newly = 0;
  const uint32_t looked = wl_expand<SSSP_SHORT, SSSP_OUT_PIECE>(
      near, ctl->ncount[p], pl, ctl->npieces[p], out_ptr, [&](int32_t v, bool) { return dist[v]; },   // (read once per vertex)
      [&](int32_t j, uint32_t d) {
        newly += sssp_try(ctl, q, f, out_row[j], __float_as_uint(__uint_as_float(d) + __uint_as_float(out_w[j])), thr, tag, dist,
                          stamp, out_ptr, near_next, pl_next, far);
      });
  wl_block_part(part, looked, newly);
}

// Closes round R (slot k of the batch); R = -1 closes sssp_init.  One workgroup sums the WlParts (no atomics on one
// word: they retire about 6 ns apart, see frontier_detect) and its first lane turns the page.
__global__ __launch_bounds__(WL_BS) void sssp_decide(SsspCtl *ctl, int k, int R, int nparts, const WlPart *__restrict__ part) {
  if (!wl_from_thread0(R < 0 || ctl->round == R)) return;
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
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t a = sums.a, b = sums.b;
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
// not their start value any more (wl_rows_min: the host fills pred with -1 first).
__global__ __launch_bounds__(WL_BS) void sssp_preds(int32_t rows, const uint32_t *__restrict__ x0, const uint32_t *__restrict__ dist,
                                                    const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_col,
                                                    const uint32_t *__restrict__ in_w, const WlPiece *__restrict__ rpieces,
                                                    int32_t n_rpieces, int32_t *pred) {
  wl_rows_min<SSSP_SHORT, SSSP_ROW_PIECE>(
      rows, in_ptr, in_col, rpieces, n_rpieces, pred,
      [&](int32_t r, uint32_t *want) { *want = dist[r]; return *want != sssp_start_bits(x0[r]); },
      [&](int32_t j, uint32_t want) { return __float_as_uint(__uint_as_float(dist[in_col[j]]) + __uint_as_float(in_w[j])) == want; });
}

} // namespace sh
