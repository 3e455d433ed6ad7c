// msbfs.hip.h -- (or,and) on packed bits (sh_bits_spmv, sh_bits_iterate): 32 * W sources per matrix read.
// The (or,and) semiring (OrAndI32, semiring.hip.h) only has the values 0 and 1, so a vertex carries W words for
// 32 * W sources: word w of vertex v is element v*W + w of an ordinary sh_vec, source s is bit s % 32 of word s / 32.
//   Out[r*W + w] = ( OR over entries e of row r with val_e != 0 and 0 <= col_e < cols of X[col_e*W + w]  &  amask )
//                | ( Y[r*W + w] & bmask )
// amask = all ones when alpha != 0, bmask likewise from beta: OrAndI32::mul / add / epilogue on every bit on its own.
// The reference runs one source per launch (app/bfs.cpp:94-174) and has no counterpart.
//
// Inputs: the CSR-stream plan's arrays and schedule, exactly what spmm_csr_kernel (multi.hip.h) takes.
//
// Lane mapping.  A lane moves LW = min(W, 4) words with one 4-, 8- or 16-byte load; Q = W / LW lanes (1, or 2 at W = 8)
// form a TEAM that fetches the 4W contiguous bytes of a column.
//   * a stream block stages ONE word per entry in LDS with coalesced 16-byte loads of col_idx and val: the column, or
//     -1 where the stored value is 0 -- `mul` is "take the word if the value is non-zero", and a column outside
//     [0, cols) already reads as 0, so the value needs no LDS of its own (17 KB instead of 34: more workgroups per CU);
//   * rows of <= MB_SHORT entries go to a GROUP of MB_G teams: team t takes entries t, t + MB_G, .. with MB_U gathers
//     in flight, so a row of up to MB_G * MB_U = 16 entries has every gather in flight at once, and the group's words
//     are folded with __shfl_xor (OR is order-free: any fold is bit-exact).  One lane per row would keep as many
//     gathers in flight per wave but walk a row sequentially, and a wave would wait for its longest row;
//   * longer rows go on an LDS list and to a whole wave, long-row segments to the workgroup, which leaves W partial
//     words per segment for msbfs_long_fixup to OR (two steps as spmm_long_fixup; no atomics on Out).
//
// Iteration (sh_bits_iterate).  changed[w] = OR over rows of (prev ^ out), folded in the wave, then in LDS, then ONE
// atomicOr per word and workgroup that has something to report.  The next launch reads these words as `live`:
// out = (new & live) | (prev & ~live).  A frozen bit changes nothing and raises nothing, so "changed of launch i" is
// "live of launch i + 1", and a launch without a live bit returns at once.  A lane whose words are all frozen gathers
// nothing.  COUNTS adds, per source, the number of rows with out & ~prev set (the vertices a BFS level reaches): one
// ballot + popcount per bit and wave of rows, lane b of a wave keeps the counts of bit b in registers, and a workgroup
// flushes at most 32 * W atomic adds.  The plain kernel (COUNTS = false) pays nothing for it.
#pragma once
#include "kernels.hip.h"

namespace sh {

struct BitsStep {
  uint32_t *changed;      // [W] device words, zero before the launch; nullptr: a plain product (no prev, live, newly)
  const uint32_t *prev;   // the previous vector (rows * W words)
  const uint32_t *live;   // [W] device words, or nullptr: every source is live
  uint32_t *newly;        // [32 * W] device words, zero before the launch (COUNTS kernels only)
};

constexpr int MB_G = 4;                          // teams per short row
constexpr int MB_U = 4, MB_UW = 2;               // gathers in flight per lane: a group's row / a wave's or workgroup's row
constexpr int MB_SHORT = 64;                     // rows up to this many entries: one group
constexpr int MB_LIST = NNZ_BLK / (MB_SHORT + 1) + 1;
constexpr int MB_PAD = BS;                       // words behind the staged entries that an unrolled read may touch (never used)

template <int LW> struct MbWords;
template <> struct MbWords<1> { using V = uint32_t; };
template <> struct MbWords<2> { using V = v2u32; };
template <> struct MbWords<4> { using V = v4u32; };

template <int LW>
__device__ __forceinline__ void mb_load(uint32_t (&w)[LW], const uint32_t *p) {
  using V = typename MbWords<LW>::V;
  const V v = *reinterpret_cast<const V *>(p);
  if constexpr (LW == 1) {
    w[0] = v;
  } else {
#pragma unroll
    for (int i = 0; i < LW; i++)
      w[i] = v[i];
  }
}
template <int LW>
__device__ __forceinline__ void mb_store(uint32_t *p, const uint32_t (&w)[LW]) {
  using V = typename MbWords<LW>::V;
  V v;
  if constexpr (LW == 1) {
    v = w[0];
  } else {
#pragma unroll
    for (int i = 0; i < LW; i++)
      v[i] = w[i];
  }
  *reinterpret_cast<V *>(p) = v;
}

// Staged entries first, first + stride, .. below hi ORed into the lane's words, U gathers in flight.
template <int W, int LW, int U>
__device__ __forceinline__ void mb_or_entries(uint32_t (&acc)[LW], const int32_t *lcol, int first, int hi, int stride,
                                              const uint32_t *__restrict__ X, int32_t cols, int q) {
  for (int j = first; j < hi; j += stride * U) {
    int32_t c[U];
    uint32_t xw[U][LW];
#pragma unroll
    for (int u = 0; u < U; u++)   // (reads past `hi` stay inside the padded array and are not used)
      c[u] = lcol[j + u * stride];
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int i = 0; i < LW; i++)
        xw[u][i] = 0u;
      if (j + u * stride < hi && (uint32_t)c[u] < (uint32_t)cols)
        mb_load<LW>(xw[u], X + (size_t)c[u] * W + LW * q);
    }
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
      for (int i = 0; i < LW; i++)
        acc[i] |= xw[u][i];
  }
}

// OR over the lanes q, q + from, q + 2 from, .. of each aligned run of `to` lanes.
template <int LW>
__device__ __forceinline__ void mb_fold(uint32_t (&acc)[LW], int from, int to) {
  for (int o = from; o < to; o <<= 1)
#pragma unroll
    for (int i = 0; i < LW; i++)
      acc[i] |= __shfl_xor(acc[i], o, 64);
}

// Per-source counts of a wave of rows.  Lane l holds the new bits of words LW * (l % QQ) .. + LW - 1 (`fin`: it holds
// any); lane b < 32 adds to cnt[w] the number of lanes whose word w has bit b set.  Called by whole waves only.
template <int W, int LW, int QQ>
__device__ __forceinline__ void mb_count(bool fin, const uint32_t (&nb)[LW], int lane, uint32_t (&cnt)[W]) {
  static_assert(LW * QQ == W, "the lanes of a team hold the W words between them");
  constexpr uint64_t EVERY = ~0ull / ((1ull << QQ) - 1ull);   // lanes 0, QQ, 2 QQ, ..
#pragma unroll
  for (int i = 0; i < LW; i++) {
    if (__ballot(fin && nb[i] != 0u) == 0ull)
      continue;
#pragma nounroll   // (unrolled, the 32 ballots are hoisted together and their SGPR pairs spill)
    for (int b = 0; b < 32; b++) {
      const uint64_t m = __ballot(fin && ((nb[i] >> b) & 1u));
#pragma unroll
      for (int qq = 0; qq < QQ; qq++) {
        const uint32_t c = (uint32_t)__popcll(m & (EVERY << qq));
        if (lane == b)
          cnt[LW * qq + i] += c;
      }
    }
  }
}

// Epilogue of row `row` for the lane's words; in an iteration also the freeze, the changed bits and the new bits.
template <int W, int LW>
__device__ __forceinline__ void mb_finish(int32_t row, const uint32_t (&acc)[LW], int q, const uint32_t *__restrict__ Y,
                                          uint32_t amask, uint32_t bmask, uint32_t *__restrict__ Out, const BitsStep &st,
                                          const uint32_t (&lv)[LW], uint32_t (&chg)[LW], uint32_t (&nb)[LW]) {
  const size_t at = (size_t)row * W + LW * q;
  uint32_t yw[LW], pw[LW], ow[LW];
#pragma unroll
  for (int i = 0; i < LW; i++)
    yw[i] = pw[i] = 0u;
  if (bmask)
    mb_load<LW>(yw, Y + at);
  if (st.changed)
    mb_load<LW>(pw, st.prev + at);
#pragma unroll
  for (int i = 0; i < LW; i++) {
    uint32_t o = (acc[i] & amask) | (yw[i] & bmask);
    if (st.changed) {
      o = (o & lv[i]) | (pw[i] & ~lv[i]);   // frozen bits are carried through
      chg[i] |= pw[i] ^ o;
      nb[i] = o & ~pw[i];
    }
    ow[i] = o;
  }
  mb_store<LW>(Out + at, ow);
}

template <int W>
__device__ __forceinline__ bool mb_gate_closed(const BitsStep &st) {
  if (!st.changed || !st.live)
    return false;
  uint32_t any = 0u;
#pragma unroll
  for (int w = 0; w < W; w++)
    any |= st.live[w];
  return any == 0u;
}

template <int W, bool COUNTS>
__global__ __launch_bounds__(BS) void msbfs_csr_kernel(
    CsrDev A, const uint32_t *__restrict__ X, const uint32_t *__restrict__ Y, uint32_t amask, uint32_t bmask,
    uint32_t *__restrict__ Out, const int32_t *__restrict__ blk_row, int32_t n_stream,
    const LongSeg *__restrict__ segs, uint32_t *__restrict__ partial, BitsStep st) {
  static_assert(W == 1 || W == 2 || W == 4 || W == 8, "1, 2, 4 or 8 words per vertex");
  constexpr int LW = W < 4 ? W : 4;     // words per lane
  constexpr int Q = W / LW;             // lanes per team
  constexpr int GL = MB_G * Q;          // lanes per group
  constexpr int GROUPS = BS / GL;       // groups per workgroup
  constexpr int TEAMS = BS / Q;         // teams per workgroup
  constexpr int WTEAMS = 64 / Q;        // teams per wave
  static_assert((MB_U - 1) * MB_G <= MB_PAD && (MB_UW - 1) * TEAMS <= MB_PAD, "unrolled reads stay inside the padded array");
  if (mb_gate_closed<W>(st))
    return;
  __shared__ __attribute__((aligned(16))) int32_t lcol[NNZ_BLK + MB_PAD];
  __shared__ int32_t rp[ROWS_BLK + 1];
  __shared__ uint16_t lst[MB_LIST];
  __shared__ int32_t n_listed;
  __shared__ uint32_t wred[BS / 64][W];
  __shared__ uint32_t lchg[W];
  __shared__ uint32_t lcnt[COUNTS ? 32 * W : 1];
  const int tid = threadIdx.x;
  const int q = tid % Q, team = tid / Q, lane = tid & 63;
  const int group = tid / GL, sub = (tid % GL) / Q;
  const int b = blockIdx.x;
  uint32_t lv[LW], chg[LW], cnt[W];
#pragma unroll
  for (int i = 0; i < LW; i++)
    lv[i] = ~0u, chg[i] = 0u;
#pragma unroll
  for (int w = 0; w < W; w++)
    cnt[w] = 0u;
  if (st.changed && st.live)
    mb_load<LW>(lv, st.live + LW * q);
  bool any_live = false;   // (a lane of frozen words only gathers nothing)
#pragma unroll
  for (int i = 0; i < LW; i++)
    any_live |= lv[i] != 0u;
  if (st.changed) {
    if (tid < W)
      lchg[tid] = 0u;
    if (COUNTS)
      for (int i = tid; i < 32 * W; i += BS)
        lcnt[i] = 0u;
  }
  // entries [from, to) of the matrix -> lcol[0 ..): the column, or -1 for a stored zero; `from` 16-byte aligned
  auto stage = [&](int from, int to) {
#pragma unroll
    for (int k = 0; k < NNZ_BLK / (BS * 4); k++) {
      const int i = from + (k * BS + tid) * 4;
      if (i < to) {
        int4 c = *reinterpret_cast<const int4 *>(A.col_idx + i);
        const uint4 v = *reinterpret_cast<const uint4 *>(A.val + i);
        c.x = v.x ? c.x : -1;
        c.y = v.y ? c.y : -1;
        c.z = v.z ? c.z : -1;
        c.w = v.w ? c.w : -1;
        *reinterpret_cast<int4 *>(&lcol[i - from]) = c;
      }
    }
  };

  if (b < n_stream) {
    // ------------------------------------------------------------ stream block
    const int2 rr = reinterpret_cast<const int2 *>(blk_row)[b];   // (first row, one-past-last row)
    const int r0 = rr.x;
    const int nr = rr.y - r0;
    if (tid == 0)
      n_listed = 0;
    for (int i = tid; i <= nr; i += BS)
      rp[i] = A.row_ptr[r0 + i];
    __syncthreads();
    const int e = rp[nr];
    const int base = rp[0] & ~3;      // 16-byte aligned start; e - base <= NNZ_BLK by construction
    stage(base, e);
    __syncthreads();
    for (int rbase = 0; rbase < nr; rbase += GROUPS) {   // (the same trips for every lane of a wave: mb_count needs whole waves)
      const int row = rbase + group;
      bool mine = row < nr;
      int lo = 0, hi = 0;
      if (mine) {
        lo = rp[row] - base, hi = rp[row + 1] - base;
        if (hi - lo > MB_SHORT) {
          if (sub == 0 && q == 0)
            lst[atomicAdd(&n_listed, 1)] = (uint16_t)row;
          mine = false;
        }
      }
      uint32_t acc[LW], nb[LW];
#pragma unroll
      for (int i = 0; i < LW; i++)
        acc[i] = nb[i] = 0u;
      if (mine && any_live)
        mb_or_entries<W, LW, MB_U>(acc, lcol, lo + sub, hi, MB_G, X, A.cols, q);
      mb_fold<LW>(acc, Q, GL);
      const bool fin = mine && sub == 0;
      if (fin)
        mb_finish<W, LW>(r0 + row, acc, q, Y, amask, bmask, Out, st, lv, chg, nb);
      if (COUNTS)
        mb_count<W, LW, Q>(fin, nb, lane, cnt);
    }
    __syncthreads();
    const int n = n_listed;
    for (int idx = tid >> 6; idx < n; idx += BS / 64) {   // one listed row per wave and trip
      const int row = lst[idx];
      const int lo = rp[row] - base, hi = rp[row + 1] - base;
      uint32_t acc[LW], nb[LW];
#pragma unroll
      for (int i = 0; i < LW; i++)
        acc[i] = nb[i] = 0u;
      if (any_live)
        mb_or_entries<W, LW, MB_UW>(acc, lcol, lo + lane / Q, hi, WTEAMS, X, A.cols, q);
      mb_fold<LW>(acc, Q, 64);
      const bool fin = lane < Q;
      if (fin)
        mb_finish<W, LW>(r0 + row, acc, q, Y, amask, bmask, Out, st, lv, chg, nb);
      if (COUNTS)
        mb_count<W, LW, Q>(fin, nb, lane, cnt);
    }
  } else {
    // ------------------------------------------------------- long-row segment
    const LongSeg sg = segs[b - n_stream];
    const int s = sg.s, e = sg.e;
    uint32_t acc[LW];
#pragma unroll
    for (int i = 0; i < LW; i++)
      acc[i] = 0u;
    for (int c0 = s & ~3; c0 < e; c0 += NNZ_BLK) {
      const int c1 = min(c0 + NNZ_BLK, e);
      stage(c0, c1);
      __syncthreads();
      if (any_live)
        mb_or_entries<W, LW, MB_UW>(acc, lcol, max(s, c0) - c0 + team, c1 - c0, TEAMS, X, A.cols, q);
      __syncthreads();
    }
    mb_fold<LW>(acc, Q, 64);
    if (lane < Q) {
#pragma unroll
      for (int i = 0; i < LW; i++)
        wred[tid >> 6][LW * q + i] = acc[i];
    }
    __syncthreads();
    if (tid < W) {
      uint32_t t = wred[0][tid];
#pragma unroll
      for (int w = 1; w < BS / 64; w++)
        t |= wred[w][tid];
      partial[(size_t)sg.slot * W + tid] = t;
    }
  }
  if (!st.changed)
    return;
  // ------------------------------------------- what the workgroup reports: wave, then LDS, then one atomic per word
  mb_fold<LW>(chg, Q, 64);
  if (lane < Q) {
#pragma unroll
    for (int i = 0; i < LW; i++)
      if (chg[i])
        atomicOr(&lchg[LW * q + i], chg[i]);
  }
  if (COUNTS && lane < 32) {
#pragma unroll
    for (int w = 0; w < W; w++)
      if (cnt[w])
        atomicAdd(&lcnt[w * 32 + lane], cnt[w]);
  }
  __syncthreads();
  if (tid < W && lchg[tid])
    atomicOr(&st.changed[tid], lchg[tid]);
  if (COUNTS)
    for (int i = tid; i < 32 * W; i += BS)
      if (lcnt[i])
        atomicAdd(&st.newly[i], lcnt[i]);
}

// OR the segment partials of each long row and finish it: one thread per (long row, word), 64 per workgroup.
template <int W, bool COUNTS>
__global__ __launch_bounds__(64) void msbfs_long_fixup(
    const LongRow *__restrict__ rows, int32_t n_long, const uint32_t *__restrict__ partial,
    const uint32_t *__restrict__ Y, uint32_t amask, uint32_t bmask, uint32_t *__restrict__ Out, BitsStep st) {
  if (mb_gate_closed<W>(st))
    return;
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool fin = i < n_long * W;
  const int w = lane % W;             // == i % W: 64 is a multiple of W
  uint32_t lv[1] = {~0u}, chg[1] = {0u}, nb[1] = {0u}, cnt[W];
#pragma unroll
  for (int k = 0; k < W; k++)
    cnt[k] = 0u;
  if (st.changed && st.live)
    lv[0] = st.live[w];
  if (fin) {
    const LongRow lr = rows[i / W];
    uint32_t acc[1] = {0u};
    for (int k = 0; k < lr.nslots; k++)
      acc[0] |= partial[(size_t)(lr.slot0 + k) * W + w];
    // (a row of W one-word "teams": word w of the row sits at row * W + w)
    mb_finish<W, 1>(lr.row, acc, w, Y, amask, bmask, Out, st, lv, chg, nb);
  }
  if (!st.changed)
    return;
  if (COUNTS) {
    mb_count<W, 1, W>(fin, nb, lane, cnt);
    if (lane < 32) {
#pragma unroll
      for (int k = 0; k < W; k++)
        if (cnt[k])
          atomicAdd(&st.newly[k * 32 + lane], cnt[k]);
    }
  }
  mb_fold<1>(chg, W, 64);
  if (lane < W && chg[0])
    atomicOr(&st.changed[lane], chg[0]);
}

// bit `source` of B[i*W + source/32] := (v[i] != 0), the other bits untouched / v[i] := that bit as int32 0 or 1
__global__ __launch_bounds__(BS) void msbfs_pack_column(const uint32_t *__restrict__ v, int64_t n, int32_t words, int32_t source,
                                                        uint32_t *__restrict__ B) {
  const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n)
    return;
  const uint32_t bit = 1u << (source & 31);
  uint32_t *p = B + i * words + (source >> 5);
  *p = v[i] ? (*p | bit) : (*p & ~bit);
}
__global__ __launch_bounds__(BS) void msbfs_unpack_column(const uint32_t *__restrict__ B, int64_t n, int32_t words, int32_t source,
                                                          uint32_t *__restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
  if (i >= n)
    return;
  v[i] = (B[i * words + (source >> 5)] >> (source & 31)) & 1u;
}

} // namespace sh
