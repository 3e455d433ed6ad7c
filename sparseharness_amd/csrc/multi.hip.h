// multi.hip.h -- K vectors per launch (sh_spmm, sh_iterate_multi): the CSR-stream plan's arrays and schedule, read ONCE
// for K interleaved vectors (element i of vector j at word i*K + j; K in {4, 8, 16, 32}):
//   Out[r*K + j] = epilogue( (+)_e  mul( X[col_e*K + j], val_e ),  alpha,  Y[r*K + j],  beta )
// The reference multiplies by one vector per launch (example/<algo>/kernel*.json:3) and has no counterpart.
//
// Lane mapping.  Q = K/4 adjacent lanes form a TEAM; lane q of a team owns vectors 4q..4q+3 and keeps four accumulators.
// The gather of a column is one 16-byte load per lane at X + (col*K + 4q) words, so a team fetches the 4K contiguous
// bytes of that column: 16 B at K = 4, a whole 128-byte line at K = 32.  The matrix stream is read once per launch:
//   * a stream block (the schedule of spmv_csr_kernel: <= NNZ_BLK entries, <= ROWS_BLK rows) stages its col_idx / val
//     words in LDS with coalesced 16-byte loads -- not its products as the one-vector kernel does: they would be K
//     times as many -- and the teams then read them from there (an LDS broadcast inside a team, no global re-load);
//   * rows of <= MM_SHORT entries are summed by ONE team, sequentially in stored order, no cross-lane step at all;
//   * longer rows go on an LDS list and are summed by a whole wave: its 64/Q teams take the entries round-robin and
//     the partial sums are folded across the teams with a __shfl_xor butterfly of strides Q, 2Q, .. 32;
//   * a long-row segment (SEG_NNZ entries) is summed by the whole workgroup, a staged chunk at a time, and leaves K
//     partials that spmm_long_fixup combines in segment order (deterministic, no float atomics).
// Column indices outside [0, cols) read as the identity for every vector (gather_x's bounds ladder).
// -ffp-contract=off as everywhere: mul and add stay two roundings.
//
// Iteration (sh_iterate_multi): flags[j] is set when a row of column j fails the convergence test.  A launch reads
// the flag words of the launch before it as `active`: a column whose word is 0 has converged -- it is FROZEN and
// carried through (out = prev) -- and a launch with no live column returns at once, which is how launches enqueued
// ahead of the host end the loop.  A frozen column raises no flag, so flags of launch i = live columns of launch i + 1.
#pragma once
#include "kernels.hip.h"

namespace sh {

struct MultiStep {
  int32_t *flags;          // [K] device words, zero before the launch; nullptr: no convergence test, no frozen columns
  const uint32_t *prev;    // the previous vectors (rows * K words): row r, column j compares prev[r*K + j]
  double delta;
  const int32_t *active;   // [K] device words, or nullptr: every column is live
};

constexpr int MM_SHORT = 16;                             // rows up to this many entries: one team, sequentially
constexpr int MM_LIST = NNZ_BLK / (MM_SHORT + 1) + 1;    // longer rows of one stream block at most
constexpr int MM_PAD = BS;                               // words behind the staged entries that an unrolled read may touch (never used)
constexpr int MM_U = 4, MM_UW = 2;                       // gathers in flight per lane: a team's row / a wave's row

template <class SR, int K>
__device__ __forceinline__ v4u32 mm_gather(const uint32_t *__restrict__ X, int32_t c, int32_t cols, int q) {
  v4u32 w = {SR::identity_bits, SR::identity_bits, SR::identity_bits, SR::identity_bits};
  if ((uint32_t)c < (uint32_t)cols)
    w = *reinterpret_cast<const v4u32 *>(X + (size_t)c * K + 4 * q);
  return w;
}

template <class SR>
__device__ __forceinline__ void mm_add(typename SR::T (&acc)[4], const v4u32 xw, uint32_t vbits) {
  using T = typename SR::T;
  const T v = from_bits<T>(vbits);
#pragma unroll
  for (int i = 0; i < 4; i++)
    acc[i] = SR::add(acc[i], SR::mul(from_bits<T>(xw[i]), v));
}

// Staged entries first, first + stride, .. below hi into the lane's accumulators, U gathers in flight.
template <class SR, int K, int U>
__device__ __forceinline__ void mm_sum_entries(typename SR::T (&acc)[4], const int32_t *lcol, const uint32_t *lval, int first, int hi, int stride,
                                               const uint32_t *__restrict__ X, int32_t cols, int q) {
  for (int j = first; j < hi; j += stride * U) {
    int32_t c[U];
    uint32_t v[U];
    v4u32 xw[U];
#pragma unroll
    for (int u = 0; u < U; u++) {   // (reads past `hi` stay inside the padded arrays and are not used)
      c[u] = lcol[j + u * stride];
      v[u] = lval[j + u * stride];
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (j + u * stride < hi)
        xw[u] = mm_gather<SR, K>(X, c[u], cols, q);
#pragma unroll
    for (int u = 0; u < U; u++)
      if (j + u * stride < hi)
        mm_add<SR>(acc, xw[u], v[u]);
  }
}

// Sum over the teams of a wave: afterwards every lane holds the total of its four vectors.
template <class SR, int K>
__device__ __forceinline__ void mm_fold_wave(typename SR::T (&acc)[4]) {
  using T = typename SR::T;
#pragma unroll
  for (int o = K / 4; o < 64; o <<= 1)
#pragma unroll
    for (int i = 0; i < 4; i++)
      acc[i] = SR::add(acc[i], from_bits<T>(__shfl_xor(to_bits<T>(acc[i]), o, 64)));
}

// The lane's live words: 1 per vector it owns that is still iterating (all 1 outside an iteration loop).
template <int K>
__device__ __forceinline__ v4u32 mm_live(const MultiStep &st, int q) {
  v4u32 a = {1u, 1u, 1u, 1u};
  if (st.flags && st.active) {
    const int4 w = *reinterpret_cast<const int4 *>(st.active + 4 * q);
    a = v4u32{w.x != 0, w.y != 0, w.z != 0, w.w != 0};
  }
  return a;
}
template <int K>
__device__ __forceinline__ bool mm_gate_closed(const MultiStep &st) {
  if (!st.flags || !st.active)
    return false;
  int any = 0;
#pragma unroll
  for (int j = 0; j < K; j++)
    any |= st.active[j];
  return any == 0;
}

// Epilogue of row `row` for the lane's four vectors: one 16-byte read of y (and of prev), one 16-byte store.
template <class SR, int K>
__device__ __forceinline__ void mm_finish(int32_t row, const typename SR::T (&acc)[4], int q, const uint32_t *__restrict__ Y,
                                          typename SR::T alpha, typename SR::T beta, bool use_y, uint32_t *__restrict__ Out,
                                          const MultiStep &st, const v4u32 live) {
  using T = typename SR::T;
  const size_t at = (size_t)row * K + 4 * q;
  v4u32 yw = {SR::identity_bits, SR::identity_bits, SR::identity_bits, SR::identity_bits}, pw = {0u, 0u, 0u, 0u}, ow;
  if (use_y)
    yw = *reinterpret_cast<const v4u32 *>(Y + at);
  if (st.flags)
    pw = *reinterpret_cast<const v4u32 *>(st.prev + at);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    T o = SR::epilogue(acc[i], alpha, from_bits<T>(yw[i]), beta, use_y);
    if (st.flags) {
      if (!live[i])
        o = from_bits<T>(pw[i]);   // frozen: carried through
      else if (SR::differs(from_bits<T>(pw[i]), o, st.delta))
        st.flags[4 * q + i] = 1;   // benign race: every writer stores 1
    }
    ow[i] = to_bits<T>(o);
  }
  *reinterpret_cast<v4u32 *>(Out + at) = ow;
}

template <class SR, int K>
__global__ __launch_bounds__(BS) void spmm_csr_kernel(
    CsrDev A, const uint32_t *__restrict__ X, const uint32_t *__restrict__ Y,
    typename SR::T alpha, typename SR::T beta, int use_y_i, uint32_t *__restrict__ Out,
    const int32_t *__restrict__ blk_row, int32_t n_stream,
    const LongSeg *__restrict__ segs, uint32_t *__restrict__ partial, MultiStep st) {
  using T = typename SR::T;
  static_assert(K == 4 || K == 8 || K == 16 || K == 32, "a team is K/4 lanes of one wave");
  constexpr int Q = K / 4;          // lanes per team
  constexpr int TEAMS = BS / Q;     // teams per workgroup
  constexpr int WTEAMS = 64 / Q;    // teams per wave
  if (mm_gate_closed<K>(st))
    return;
  static_assert((MM_U - 1) <= MM_PAD && (MM_UW - 1) * TEAMS <= MM_PAD, "unrolled reads stay inside the padded arrays");
  __shared__ __attribute__((aligned(16))) int32_t lcol[NNZ_BLK + MM_PAD];
  __shared__ __attribute__((aligned(16))) uint32_t lval[NNZ_BLK + MM_PAD];
  __shared__ int32_t rp[ROWS_BLK + 1];
  __shared__ uint16_t lst[MM_LIST];
  __shared__ int32_t n_listed;
  __shared__ uint32_t wred[BS / 64][K];
  const int tid = threadIdx.x;
  const int q = tid % Q, team = tid / Q, lane = tid & 63;
  const bool use_y = use_y_i != 0;
  const int b = blockIdx.x;
  const v4u32 live = mm_live<K>(st, q);
  const bool any_live = (live[0] | live[1] | live[2] | live[3]) != 0u;   // (a lane of frozen vectors only gathers nothing)
  // entries [from, to) of the matrix -> lcol / lval[0 ..), `from` 16-byte aligned, to - from <= NNZ_BLK
  auto stage = [&](int from, int to) {
#pragma unroll
    for (int k = 0; k < NNZ_BLK / (BS * 4); k++) {
      const int i = from + (k * BS + tid) * 4;
      if (i < to) {
        *reinterpret_cast<int4 *>(&lcol[i - from]) = *reinterpret_cast<const int4 *>(A.col_idx + i);
        *reinterpret_cast<uint4 *>(&lval[i - from]) = *reinterpret_cast<const uint4 *>(A.val + i);
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
    for (int row = team; row < nr; row += TEAMS) {
      const int lo = rp[row] - base, hi = rp[row + 1] - base;
      if (hi - lo > MM_SHORT) {
        if (q == 0)
          lst[atomicAdd(&n_listed, 1)] = (uint16_t)row;
        continue;
      }
      T acc[4] = {SR::identity(), SR::identity(), SR::identity(), SR::identity()};
      if (any_live)
        mm_sum_entries<SR, K, MM_U>(acc, lcol, lval, lo, hi, 1, X, A.cols, q);
      mm_finish<SR, K>(r0 + row, acc, q, Y, alpha, beta, use_y, Out, st, live);
    }
    __syncthreads();
    const int n = n_listed;
    for (int idx = tid >> 6; idx < n; idx += BS / 64) {   // one listed row per wave and trip
      const int row = lst[idx];
      const int lo = rp[row] - base, hi = rp[row + 1] - base;
      T acc[4] = {SR::identity(), SR::identity(), SR::identity(), SR::identity()};
      if (any_live)
        mm_sum_entries<SR, K, MM_UW>(acc, lcol, lval, lo + lane / Q, hi, WTEAMS, X, A.cols, q);
      mm_fold_wave<SR, K>(acc);
      if (lane < Q)
        mm_finish<SR, K>(r0 + row, acc, q, Y, alpha, beta, use_y, Out, st, live);
    }
  } else {
    // ------------------------------------------------------- long-row segment
    const LongSeg sg = segs[b - n_stream];
    const int s = sg.s, e = sg.e;
    T acc[4] = {SR::identity(), SR::identity(), SR::identity(), SR::identity()};
    for (int c0 = s & ~3; c0 < e; c0 += NNZ_BLK) {
      const int c1 = min(c0 + NNZ_BLK, e);
      stage(c0, c1);
      __syncthreads();
      if (any_live)
        mm_sum_entries<SR, K, MM_UW>(acc, lcol, lval, max(s, c0) - c0 + team, c1 - c0, TEAMS, X, A.cols, q);
      __syncthreads();
    }
    mm_fold_wave<SR, K>(acc);
    if (lane < Q) {
#pragma unroll
      for (int i = 0; i < 4; i++)
        wred[tid >> 6][4 * q + i] = to_bits<T>(acc[i]);
    }
    __syncthreads();
    if (tid < K) {
      T t = from_bits<T>(wred[0][tid]);
#pragma unroll
      for (int w = 1; w < BS / 64; w++)
        t = SR::add(t, from_bits<T>(wred[w][tid]));
      partial[(size_t)sg.slot * K + tid] = to_bits<T>(t);
    }
  }
}

// Combine the segment partials of each long row in segment order: one thread per (long row, vector).
template <class SR, int K>
__global__ __launch_bounds__(64) void spmm_long_fixup(
    const LongRow *__restrict__ rows, int32_t n_long, const uint32_t *__restrict__ partial,
    const uint32_t *__restrict__ Y, typename SR::T alpha, typename SR::T beta, int use_y_i,
    uint32_t *__restrict__ Out, MultiStep st) {
  using T = typename SR::T;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_long * K || mm_gate_closed<K>(st))
    return;
  const LongRow lr = rows[i / K];
  const int j = i % K;
  const bool use_y = use_y_i != 0;
  T acc = SR::identity();
  for (int k = 0; k < lr.nslots; k++)
    acc = SR::add(acc, from_bits<T>(partial[(size_t)(lr.slot0 + k) * K + j]));
  const size_t at = (size_t)lr.row * K + j;
  T o = SR::epilogue(acc, alpha, use_y ? from_bits<T>(Y[at]) : SR::identity(), beta, use_y);
  if (st.flags) {
    const T in = from_bits<T>(st.prev[at]);
    if (st.active && st.active[j] == 0)
      o = in;
    else if (SR::differs(in, o, st.delta))
      st.flags[j] = 1;
  }
  Out[at] = to_bits<T>(o);
}

} // namespace sh
