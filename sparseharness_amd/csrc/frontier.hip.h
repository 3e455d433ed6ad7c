// frontier.hip.h -- kernels of sh_iterate_frontier: an iteration loop that recomputes only the rows whose inputs
// changed in the launch before (DESIGN.md "Frontier-driven iteration").
//
// From launch 1 on sh_iterate runs out = kernel(in, y = in), so row r of launch k reads x_k[col_j] for its entries j
// and x_k[r]; if none of those words changed between x_{k-1} and x_k the row's word does not change either.  With
//   C_k = { i : bits(x_k[i]) != bits(x_{k-1}[i]) }        (the changed list)
//   active_k = C_k  u  { r : row r has an entry with 0 <= col < cols and col in C_k }
// a SPARSE launch recomputes the rows of active_k only, in place:
//   frontier_mark   walks the transposed pattern (col_ptr / row_of) of every column of C_k and claims the rows (one
//                   stamp word per row holding the launch's number, claimed by atomic exchange) into the active list;
//   frontier_pull   SR's reduction over the CSR entries of every active row -> side[i] (the row's raw "dot");
//   frontier_apply  epilogue with y = x[r]; writes the words that differ, appends them to the next changed list, adds up
//                   their transposed-column lengths (what dense_share is compared with), raises the `differs` flag.
// Nothing of x is written before every active row is computed (pull and apply are two kernels), so the launch keeps
// sh_iterate's Jacobi semantics.  A DENSE launch is sh_iterate's own (any plan), followed by frontier_detect, which
// builds the changed list by comparing in / out over all rows.  frontier_decide closes every launch: it records what
// the launch did and opens or closes the gate of the next one (see FrontierCtl).
//
// min / or / max are order-free and every (min,+) product is rounded on its own, so a recomputed row has the same
// bits whatever kernel produced it.  That also makes integer atomics legal for rows cut over several waves: every
// (min,+) partial is a non-negative float, whose order is that of its bit pattern as an unsigned word.
//
// Work distribution as worklist.hip.h describes it, with FR_SHORT and FR_COL_PIECE (mark) / FR_ROW_PIECE (pull).  The
// transposed pattern is built once per handle by wl_col_hist / wl_transpose_scatter.
#pragma once
#include "kernels.hip.h"
#include "worklist.hip.h"

namespace sh {

constexpr int FR_SHORT = 8;           // rows / columns up to this many entries: one lane each
constexpr int FR_COL_PIECE = 2048;    // transposed columns above this are marked in pieces of this many entries
constexpr int FR_ROW_PIECE = 4096;    // rows above the schedule's long-row threshold are pulled in pieces of this many entries
constexpr int FR_BATCH = 8;           // launches enqueued ahead of the host (as sh_iterate's ITER_BATCH)
constexpr int FR_CTL_BYTES = 512;     // device bytes set aside for FrontierCtl

struct FrontierRec {   // what launch k of a batch did (read back by the host once per batch)
  int32_t ran, differs, sparse_next;
  uint32_t changed, active;
};
// Control block in device memory.  Launch L (counted over the whole call) consumes the changed list whose length is
// ccount[L & 1] and produces the one of ccount[(L + 1) & 1]; both live in the same storage (mark has consumed the old
// list before apply / detect write the new one).
struct FrontierCtl {
  uint32_t ccount[2], centries[2], cpieces[2];
  uint32_t acount, rpieces;       // active rows / long-row pieces of the sparse launch in flight
  int32_t go[FR_BATCH + 1];       // go[k] != 0: launch k of the batch runs (its kernels return at once otherwise)
  int32_t flag[FR_BATCH];         // SR::differs raised by launch k (what ends the loop)
  FrontierRec rec[FR_BATCH];
};
// (a WlPiece's id is a column for mark and an active-list slot for pull)

// a changed row joins the next changed list: its place, its transposed column's length, its pieces when the column is long
__device__ __forceinline__ uint32_t fr_push_changed(FrontierCtl *ctl, int p, bool changed, int32_t r, int lane,
                                                    const int32_t *__restrict__ col_ptr, uint32_t *__restrict__ clist,
                                                    WlPiece *__restrict__ cplist) {
  const uint32_t at = wl_wave_append(&ctl->ccount[p], changed, lane);
  uint32_t len = 0;
  if (changed) {
    clist[at] = (uint32_t)r;
    len = (uint32_t)(col_ptr[r + 1] - col_ptr[r]);
    wl_push_pieces<FR_COL_PIECE>(&ctl->cpieces[p], (uint32_t)r, len, cplist);
  }
  return len;
}

// ---- the loop
// Opens a batch: launch 0 runs, the others wait for frontier_decide.
__global__ void frontier_begin(FrontierCtl *ctl) {
  const int k = (int)threadIdx.x;
  if (k <= FR_BATCH) ctl->go[k] = k == 0 ? 1 : 0;
  if (k < FR_BATCH) {
    ctl->flag[k] = 0;
    ctl->rec[k] = FrontierRec{0, 0, 0, 0u, 0u};
  }
}

// After a dense launch: the rows whose bits it changed -> changed list p (the one the launch produces), its entry sum
// and long-column pieces.  A workgroup owns a contiguous run of rows and reads it twice: first it counts its changed
// rows and reserves their places with ONE add on the list cursor, then it reads the run again (out of L2) and writes
// them.  (One add per wave and 64 rows was measured first: adds on one address retire about 6 ns apart, which made this
// kernel cost 20 us on 171 K rows and 650 us on 8.4 M, twice the dense launch it follows.)
__global__ __launch_bounds__(WL_BS) void frontier_detect(FrontierCtl *ctl, int k, int p, const uint32_t *__restrict__ in,
                                                         const uint32_t *__restrict__ out, int32_t rows,
                                                         const int32_t *__restrict__ col_ptr, uint32_t *__restrict__ clist,
                                                         WlPiece *__restrict__ cplist) {
  if (ctl->go[k] == 0) return;
  __shared__ uint32_t s_cnt[WL_BS / 64], s_base;
  const int lane = wl_lane(), wave = (int)(threadIdx.x >> 6);
  const int64_t per = (((int64_t)rows + gridDim.x - 1) / gridDim.x + WL_BS - 1) / WL_BS * WL_BS;   // rows per workgroup
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(r0 + per, (int64_t)rows);
  uint32_t mine = 0;   // changed rows of this wave
  for (int64_t base = r0 + wave * 64; base < r1; base += WL_BS) {
    const int64_t r = base + lane;
    mine += (uint32_t)__popcll(__ballot(r < r1 && in[r] != out[r]));
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  uint32_t total = 0, before = 0;
  for (int w = 0; w < WL_BS / 64; w++) {
    if (w < wave) before += s_cnt[w];
    total += s_cnt[w];
  }
  if (total == 0) return;   // (uniform over the workgroup)
  if (threadIdx.x == 0) s_base = wl_add(&ctl->ccount[p], total);
  __syncthreads();
  uint32_t at = s_base + before, entries = 0;
  for (int64_t base = r0 + wave * 64; base < r1; base += WL_BS) {
    const int64_t r = base + lane;
    const bool changed = r < r1 && in[r] != out[r];
    const uint64_t m = __ballot(changed);
    if (changed) {
      clist[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)r;
      const uint32_t len = (uint32_t)(col_ptr[r + 1] - col_ptr[r]);
      entries += len;
      wl_push_pieces<FR_COL_PIECE>(&ctl->cpieces[p], (uint32_t)r, len, cplist);
    }
    at += (uint32_t)__popcll(m);
  }
  entries = wl_wave_sum(entries);
  if (lane == 0 && entries) wl_add(&ctl->centries[p], entries);
}

// A lane claims row r for the launch whose number is `gen`: whoever sees an older stamp appends the row.
__device__ __forceinline__ void fr_claim(FrontierCtl *ctl, int32_t r, uint32_t gen, const int32_t *__restrict__ row_ptr,
                                         uint32_t *__restrict__ stamp, uint32_t *__restrict__ alist, uint32_t *__restrict__ side,
                                         WlPiece *__restrict__ rplist, uint32_t identity_bits) {
  if (__hip_atomic_exchange(&stamp[r], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) return;
  const uint32_t i = wl_append_here(&ctl->acount);
  alist[i] = (uint32_t)r;
  const uint32_t len = (uint32_t)(row_ptr[r + 1] - row_ptr[r]);
  if (len > (uint32_t)FR_ROW_PIECE) side[i] = identity_bits;   // pulled in pieces that meet in side[i] by integer atomics: start from the identity
  wl_push_pieces<FR_ROW_PIECE>(&ctl->rpieces, i, len, rplist);
}

__global__ __launch_bounds__(WL_BS) void frontier_mark(FrontierCtl *ctl, int k, int p, uint32_t gen, int32_t rows,
                                                       const int32_t *__restrict__ col_ptr, const int32_t *__restrict__ row_of,
                                                       const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ clist,
                                                       const WlPiece *__restrict__ cplist, uint32_t *__restrict__ stamp,
                                                       uint32_t *__restrict__ alist, uint32_t *__restrict__ side,
                                                       WlPiece *__restrict__ rplist, uint32_t identity_bits) {
  if (ctl->go[k] == 0) return;
  const auto claim = [&](int32_t r) { fr_claim(ctl, r, gen, row_ptr, stamp, alist, side, rplist, identity_bits); };
  (void)wl_expand<FR_SHORT, FR_COL_PIECE>(
      clist, ctl->ccount[p], cplist, ctl->cpieces[p], col_ptr,
      [&](int32_t c, bool listed) { if (listed && c < rows) claim(c); return 0u; },   // the rows of C_k themselves
      [&](int32_t j, uint32_t) { claim(row_of[j]); });
}

template <class SR>
__device__ __forceinline__ typename SR::T fr_wave_reduce(typename SR::T acc) {
  for (int o = 32; o > 0; o >>= 1) acc = SR::add(acc, __shfl_xor(acc, o));
  return acc;
}
template <class SR>
__device__ __forceinline__ typename SR::T fr_entries(const CsrDev &A, const uint32_t *__restrict__ x, int32_t s, int32_t e, int32_t step) {
  using T = typename SR::T;
  T acc = SR::identity();
  for (int32_t j = s; j < e; j += step)
    acc = SR::add(acc, SR::mul(gather_x<SR>(x, A.col_idx[j], A.cols), from_bits<T>(A.val[j])));
  return acc;
}

// side[i] = the reduction over the entries of active row i (before the epilogue)
template <class SR>
__global__ __launch_bounds__(WL_BS) void frontier_pull(FrontierCtl *ctl, int k, CsrDev A, const uint32_t *__restrict__ x,
                                                       const uint32_t *__restrict__ alist, uint32_t *__restrict__ side,
                                                       const WlPiece *__restrict__ rplist) {
  using T = typename SR::T;
  if (ctl->go[k] == 0) return;
  const int lane = wl_lane();
  const int64_t n = ctl->acount, np = ctl->rpieces;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const int32_t r = valid ? (int32_t)alist[base + lane] : 0;
    const int32_t s = valid ? A.row_ptr[r] : 0;
    const int32_t len = valid ? A.row_ptr[r + 1] - s : 0;
    T mine = SR::identity();
    if (valid && len <= FR_SHORT) mine = fr_entries<SR>(A, x, s, s + len, 1);
    uint64_t m = __ballot(len > FR_SHORT && len <= FR_ROW_PIECE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const T acc = fr_wave_reduce<SR>(fr_entries<SR>(A, x, sb + lane, sb + lb, 64));
      if (lane == src) mine = acc;
    }
    if (valid && len <= FR_ROW_PIECE) side[base + lane] = to_bits<T>(mine);
  }
  for (int64_t q = wl_wave(); q < np; q += wl_waves()) {
    const WlPiece pc = rplist[q];
    const int32_t r = (int32_t)alist[pc.id];
    const int32_t s = A.row_ptr[r] + (int32_t)pc.off;
    const int32_t e = min(s + FR_ROW_PIECE, A.row_ptr[r + 1]);
    const T acc = fr_wave_reduce<SR>(fr_entries<SR>(A, x, s + lane, e, 64));
    if (lane == 0) {
      if constexpr (SR::id == 1)        // (min,+): partials are non-negative floats, ordered as their bit patterns
        __hip_atomic_fetch_min(&side[pc.id], to_bits<T>(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else if constexpr (SR::id == 2)   // (or,and): 0 / 1
        __hip_atomic_fetch_or(&side[pc.id], to_bits<T>(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else                              // (max,min) on int32
        __hip_atomic_fetch_max((int32_t *)&side[pc.id], (int32_t)acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Epilogue with y = x[r], in place: only words that differ are written (p: the changed list this launch PRODUCES).
template <class SR>
__global__ __launch_bounds__(WL_BS) void frontier_apply(FrontierCtl *ctl, int k, int p, uint32_t *__restrict__ x,
                                                        const uint32_t *__restrict__ alist, const uint32_t *__restrict__ side,
                                                        const int32_t *__restrict__ col_ptr, uint32_t *__restrict__ clist,
                                                        WlPiece *__restrict__ cplist, typename SR::T alpha, typename SR::T beta,
                                                        int use_y, double delta) {
  using T = typename SR::T;
  if (ctl->go[k] == 0) return;
  const int lane = wl_lane();
  const int64_t n = ctl->acount;
  uint32_t entries = 0;
  bool differs = false;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    int32_t r = 0;
    bool changed = false;
    if (valid) {
      r = (int32_t)alist[base + lane];
      const uint32_t old = x[r];
      const T yv = use_y ? from_bits<T>(old) : SR::identity();
      const T o = SR::epilogue(from_bits<T>(side[base + lane]), alpha, yv, beta, use_y != 0);
      changed = to_bits<T>(o) != old;
      if (changed) x[r] = to_bits<T>(o);
      differs = differs || SR::differs(from_bits<T>(old), o, delta);
    }
    entries += fr_push_changed(ctl, p, changed, r, lane, col_ptr, clist, cplist);
  }
  entries = wl_wave_sum(entries);
  if (lane == 0 && entries) wl_add(&ctl->centries[p], entries);
  if (differs) ctl->flag[k] = 1;   // benign race: every writer stores 1
}

// Closes launch k of a batch (launch L of the call, p = L & 1 the list it consumed): records what it did, chooses the
// next launch's mode and opens its gate when the loop goes on in the mode this batch was enqueued for.
__global__ void frontier_decide(FrontierCtl *ctl, int k, int p, int dense, int32_t rows, uint32_t max_entries,
                                int allow_sparse_next, int batch_sparse) {
  if (threadIdx.x != 0 || ctl->go[k] == 0) return;
  const int q = p ^ 1;
  const int sparse_next = allow_sparse_next && ctl->centries[q] <= max_entries;
  ctl->rec[k] = FrontierRec{1, ctl->flag[k], sparse_next, ctl->ccount[q], dense ? (uint32_t)rows : ctl->acount};
  ctl->go[k + 1] = (ctl->flag[k] != 0 && sparse_next == batch_sparse) ? 1 : 0;
  ctl->ccount[p] = 0; ctl->centries[p] = 0; ctl->cpieces[p] = 0;
  ctl->acount = 0; ctl->rpieces = 0;
}

} // namespace sh
