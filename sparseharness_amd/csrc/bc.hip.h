// bc.hip.h -- kernels of sh_bc: betweenness centrality by Brandes' two sweeps per source (Brandes, "A faster algorithm for
// betweenness centrality", J. Math. Sociol. 2001), every sum in float64 and in ONE FIXED ORDER, so that the scores are a
// function of the matrix and the sources alone and are compared with == (DESIGN.md "6p Betweenness centrality").
//
// The handle holds the simple directed graph under the entries twice: in_ptr / in_col (the sources c of the edges c -> r,
// by r) and out_ptr / out_col (the targets, by c), BOTH strictly ascending inside a list: the surviving entries become
// 64-bit keys (r << bits | c), sorted and deduplicated, and the flipped keys are sorted again.  The state of a source:
// level[v] (an unsigned word, 0xFFFFFFFF while unreached), sigma[v] and delta[v] (float64), order[] = the vertices in
// the order they were reached, which is its own queue, and lstart[L] = where level L starts in it.
//
// THE SUM OF A LIST (bc_list_sum) is defined once, for a list of `len` entries in ascending neighbour index whose entry
// j contributes the term t[j] (+0.0 where the entry does not take part: the wrong level):
//   the list is cut into pieces of BC_PIECE entries, the last one shorter;
//   inside a piece 64 strided partials: partial[l] = (((+0.0 + t[l]) + t[l + 64]) + t[l + 128]) + ... ;
//   the 64 partials are folded by a butterfly: for o = 32, 16, 8, 4, 2, 1: partial[l] = partial[l] + partial[l ^ o]
//   (IEEE addition commutes, so the 64 lanes hold the same bits);
//   the piece sums are added left to right, starting from +0.0.
// Every term is non-negative, so +0.0 + t == t and padding is exact: a list of up to BC_LANE = 8 entries has the sum
// ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7)), which one lane computes alone; a longer one is walked by one wave,
// piece after piece.  The three tiers (a lane, a wave, a wave over several pieces) are ONE function of the list.
//
// ONE OWNER PER VALUE.  sigma[w] is written by the one lane or wave that PULLS over w's in-list, delta[v] and bc[v] by the
// one that pulls over v's out-list; what they read was written by launches that ended before.  There is no float
// atomic, and no value depends on the queue order, the grid, the batch or the run: the queue order decides only WHO
// computes a value, never from what or in which order.  The only atomics are the unsigned minimum that claims a vertex
// (bc_expand), the list cursors, and an unsigned 64-bit maximum over the bit patterns of sigma (non-negative doubles
// order as their bits), whose result does not depend on order either.
//
// A FORWARD STEP L is three launches, gated by the control block: bc_expand pushes along the out-lists of level L =
// order[a, b): atomicMin(level[w], L + 1) claims w, and the one lane that read 0xFFFFFFFF appends it (no
// compare-and-swap); bc_count: every vertex w of the new segment order[b, tail) pulls sigma[w] = the sum over its
// in-list of sigma[v] where level[v] == L; bc_close, one workgroup, records the step and opens the next or ends the
// sweep.  THE BACKWARD SWEEP is one ungated launch per level L = depth - 1 ... 1 (level 0 is the source alone, whose
// delta is not an output): every v of segment L pulls delta[v] = the sum over its out-list of
// (sigma[v] / sigma[w]) * (1 + delta[w]) where level[w] == L + 1, and bc[v] = bc[v] + delta[v].
//
// NO KERNEL EVER WAITS for another kernel's write: every exchange crosses a launch boundary; no spin, no flag, no retry.
// EVERY LOOP IS BOUNDED by a list length, a level's width or `rows`.  Values are written with vector stores, atomics or
// plain C++ only.
//
// Worst cases.  A path: three launches forward and one backward per level and source, however narrow the level.  A hub:
// its list is pulled by one wave alone, 64 entries at a time.  sigma above 2^53 is rounded, above the float64 range it is
// +inf (grids: C(n, n/2) leaves float64 near n = 1030) and delta is then whatever IEEE gives.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int BC_LANE = 8;               // lists up to this many entries: one lane each (the butterfly's last three levels)
constexpr int BC_PIECE = 2048;           // a piece of a list: 64 strided partials and one butterfly; out-lists above it are pushed in pieces
constexpr int BC_BATCH = 32;             // steps enqueued ahead of the host at most (the first batch holds 8)
constexpr int BC_MAX_BLOCKS = 1024;      // workgroups of a launch at most: one WlPart each
constexpr int BC_CTL_BYTES = 1024;       // device bytes set aside for BcCtl
constexpr int BC_PART_BYTES = 16 * BC_MAX_BLOCKS;
constexpr uint32_t BC_NONE = 0xFFFFFFFFu;
static_assert(BC_LANE == 8, "bc_list_sum writes the last three levels of the butterfly out for eight terms");

struct BcRec {   // what step k of a batch did (read back by the host once per batch)
  int32_t ran;
  uint32_t found, edges, pad;   // the vertices of the new level; the out-list entries of the level walked
};
// Control block in device memory.  The pieces of level L's long out-lists live in piece list L & 1.
struct BcCtl {
  int32_t step;                 // the step that runs next (-1 once the forward sweep has ended)
  int32_t finished;
  uint32_t a, b;                // the level: order[a, b)
  uint32_t tail;                // where the next level ends so far (atomic cursor)
  uint32_t qpieces[2];
  int32_t depth;                // the last level that holds a vertex (set when the sweep ends)
  uint64_t smax;                // the bits of the largest sigma so far
  uint64_t pad;
  BcRec rec[BC_BATCH];
};
// The WlPart of a workgroup of bc_expand: a = out-list entries of the level.

struct BcGraph {   // the handle's lists as a kernel argument
  int32_t rows;
  const int32_t *in_ptr, *in_col, *out_ptr, *out_col;
};
struct BcState {
  uint32_t *level, *order, *lstart;   // rows, rows, rows + 1 words
  double *sigma, *delta;
  WlPiece *pl[2];
};

// ---- building the handle (once) -----------------------------------------------------------------------------------------
// pos = exclusive scan of flag (wl_und_flag: the entry counts and is no self-loop): survivor j -> key[pos[j]] = (r << bits | c)
__global__ __launch_bounds__(WL_BS) void bc_in_keys(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                     const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                     int64_t nnz, int32_t rows, int bits, uint64_t *__restrict__ key) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz && flag[j])
    key[pos[j]] = ((uint64_t)(uint32_t)wl_row_of(row_ptr, rows, j) << bits) | (uint64_t)(uint32_t)col_idx[j];
}
// Edge i of the simple graph (the first key of its run; pos = exclusive scan of head): ikey[pos[i]] = (r << bits | c), in
// sorted order still, and okey[pos[i]] = (c << bits | r), to be sorted
__global__ __launch_bounds__(WL_BS) void bc_out_keys(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                      const uint32_t *__restrict__ pos, int64_t n, int bits,
                                                      uint64_t *__restrict__ ikey, uint64_t *__restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    const uint64_t r = key[i] >> bits, c = key[i] & ((1ull << bits) - 1ull);
    ikey[pos[i]] = key[i];
    okey[pos[i]] = (c << bits) | r;
  }
}

// ---- the sum of a list ----------------------------------------------------------------------------------------------------
// The butterfly over the wave's 64 partials -> every lane (wave-uniform control flow only).  Its order is part of the
// result: it is written out here and restated by tests/bc_ref.py and host/src/bc_scores.cpp.
__device__ __forceinline__ double bc_butterfly(double v) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
// Every lane of the wave brings a list (s, len; `valid`) and a carried double; term(j, carried) is the term of entry j,
// +0.0 where the entry does not take part.  -> for the lane that brought the list, its sum as the header defines it.
// (Wave-uniform control flow only: the whole wave calls it together.)
template <class Term>
__device__ __forceinline__ double bc_list_sum(bool valid, int32_t s, int32_t len, double carried, Term term) {
  const int lane = wl_lane();
  double sum = 0.0;
  if (!valid) len = 0;
  if (len <= BC_LANE) {   // partial[l] = t[l], and the butterfly's levels 32, 16 and 8 add +0.0
    double t[BC_LANE];
#pragma unroll
    for (int k = 0; k < BC_LANE; k++) t[k] = k < len ? term(s + k, carried) : 0.0;
    sum = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
  }
  uint64_t m = __ballot(len > BC_LANE);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
    const double cb = __shfl(carried, src);
    double acc = 0.0;
    for (int32_t p0 = 0; p0 < lb; p0 += BC_PIECE) {   // the pieces, left to right
      const int32_t pe = min(lb, p0 + BC_PIECE);
      double partial = 0.0;
      for (int32_t j = p0 + lane; j < pe; j += 64) partial = partial + term(sb + j, cb);
      acc = acc + bc_butterfly(partial);
    }
    if (lane == src) sum = acc;
  }
  return sum;
}

// ---- the launches of a source ---------------------------------------------------------------------------------------------
// Nothing reached but the source (the host has zeroed the control block): it is level 0, alone, with one path.
__global__ __launch_bounds__(WL_BS) void bc_init(BcCtl *ctl, BcGraph G, BcState St, int32_t src) {
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < G.rows; v += (int64_t)gridDim.x * WL_BS) {
    const bool is_src = v == (int64_t)src;
    St.level[v] = is_src ? 0u : BC_NONE;
    St.sigma[v] = is_src ? 1.0 : 0.0;
    St.delta[v] = 0.0;
    if (is_src) {   // (one thread of the launch)
      St.order[0] = (uint32_t)src;
      St.lstart[0] = 0u; St.lstart[1] = 1u;
      ctl->a = 0u; ctl->b = 1u; ctl->tail = 1u;
      ctl->smax = (uint64_t)__double_as_longlong(1.0);
      wl_push_pieces<BC_PIECE>(&ctl->qpieces[0], (uint32_t)src, (uint32_t)(G.out_ptr[src + 1] - G.out_ptr[src]), St.pl[0]);
    }
  }
}

// Step L: the out-lists of level L are pushed; the lane whose atomic minimum read an unreached word owns w and appends it.
__global__ __launch_bounds__(WL_BS) void bc_expand(BcCtl *ctl, int L, BcGraph G, BcState St, WlPart *__restrict__ part) {
  if (ctl->step != L) return;
  const int p = L & 1, q = p ^ 1;
  const uint32_t a = ctl->a, next = (uint32_t)L + 1u;
  const uint32_t looked = wl_expand<BC_LANE, BC_PIECE>(
      St.order + a, (int64_t)(ctl->b - a), St.pl[p], (int64_t)ctl->qpieces[p], G.out_ptr, [](int32_t, bool) { return 0u; },
      [&](int32_t j, uint32_t) {
        const uint32_t w = (uint32_t)G.out_col[j];
        if (wl_load(&St.level[w]) != BC_NONE || wl_umin(&St.level[w], next) != BC_NONE) return;
        St.order[wl_append_here(&ctl->tail)] = w;
        wl_push_pieces<BC_PIECE>(&ctl->qpieces[q], w, (uint32_t)(G.out_ptr[w + 1] - G.out_ptr[w]), St.pl[q]);
      });
  wl_block_part(part, looked, 0u);
}

// Step L: sigma[w] for every vertex w of the new segment order[b, tail), pulled over its in-list.
__global__ __launch_bounds__(WL_BS) void bc_count(BcCtl *ctl, int L, BcGraph G, BcState St) {
  if (ctl->step != L) return;
  const int lane = wl_lane();
  const int64_t b = (int64_t)ctl->b, tail = (int64_t)ctl->tail;
  const uint32_t from = (uint32_t)L;
  uint64_t top = 0;
  for (int64_t base = b + wl_wave() * 64; base < tail; base += wl_waves() * 64) {
    const bool valid = base + lane < tail;
    const int32_t w = valid ? (int32_t)St.order[base + lane] : 0;
    const int32_t s = valid ? G.in_ptr[w] : 0;
    const int32_t len = valid ? G.in_ptr[w + 1] - s : 0;
    const double sum = bc_list_sum(valid, s, len, 0.0, [&](int32_t j, double) {
      const int32_t v = G.in_col[j];
      return St.level[v] == from ? St.sigma[v] : 0.0;   // (neither is written in this launch for a vertex of level L)
    });
    if (valid) {
      St.sigma[w] = sum;
      top = max(top, (uint64_t)__double_as_longlong(sum));
    }
  }
  top = wl_wave_fold<WlMax>(top);
  if (lane == 0 && top > wl_load(&ctl->smax)) (void)__hip_atomic_fetch_max(&ctl->smax, top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Closes step L (slot k of the batch).  One workgroup folds the WlParts and its first thread records the step and decides.
__global__ __launch_bounds__(WL_BS) void bc_close(BcCtl *ctl, int k, int L, int nparts, const WlPart *__restrict__ part, BcState St) {
  if (!wl_from_thread0(ctl->step == L)) return;
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t b = ctl->b, tail = ctl->tail;
  ctl->rec[k] = BcRec{1, tail - b, sums.a, 0u};
  ctl->qpieces[L & 1] = 0u;
  if (tail == b) { ctl->depth = L; ctl->finished = 1; ctl->step = -1; return; }
  St.lstart[L + 2] = tail;   // level L + 1 = order[b, tail)
  ctl->a = b; ctl->b = tail;
  ctl->step = L + 1;
}

// Level L of the backward sweep (ungated: the host knows the depth): delta[v] for every v of the level, pulled over its
// out-list, and bc[v] = bc[v] + delta[v].  (L >= 1: the source is not in it.)
__global__ __launch_bounds__(WL_BS) void bc_delta(int L, BcGraph G, BcState St, double *__restrict__ bc) {
  const int lane = wl_lane();
  const int64_t a = (int64_t)St.lstart[L], b = (int64_t)St.lstart[L + 1];
  const uint32_t below = (uint32_t)L + 1u;
  for (int64_t base = a + wl_wave() * 64; base < b; base += wl_waves() * 64) {
    const bool valid = base + lane < b;
    const int32_t v = valid ? (int32_t)St.order[base + lane] : 0;
    const int32_t s = valid ? G.out_ptr[v] : 0;
    const int32_t len = valid ? G.out_ptr[v + 1] - s : 0;
    const double sum = bc_list_sum(valid, s, len, valid ? St.sigma[v] : 0.0, [&](int32_t j, double sigma_v) {
      const int32_t w = G.out_col[j];
      return St.level[w] == below ? (sigma_v / St.sigma[w]) * (1.0 + St.delta[w]) : 0.0;   // (delta[w]: written by the launch before)
    });
    if (valid) {
      St.delta[v] = sum;
      bc[v] = bc[v] + sum;
    }
  }
}

} // namespace sh
