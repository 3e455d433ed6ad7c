// trsv.hip.h -- kernels of sh_trsv: the sparse triangular solve T x = b by LEVEL SETS (Anderson, Saad, "Solving sparse
// triangular linear systems on parallel computers", Int. J. High Speed Computing 1989; Naumov, "Parallel solution of
// sparse triangular linear systems in the preconditioned iterative methods on the GPU", NVIDIA NVR-2011-001), in float64
// and in ONE FIXED ORDER, so that x is a function of the matrix and b alone and is compared with == (DESIGN.md "6q Sparse
// triangular solve").
//
// The handle holds, for every row r, THE LIST of its strictly-triangular entries in ascending (column, position as given)
// -- ptr / col / val, parallel entries separate terms -- and d[r], its diagonal entries widened to float64 and added
// left to right from +0.0.  The entries that take part become 64-bit keys (r << bits | c) with the value riding along,
// sorted by a stable radix sort.  level[r] = 0 for an empty list, else 1 + the largest level in the list; order[] = the
// rows in ascending (level, index), lstart[L] = where level L starts in it.
//
// THE ANALYSIS (once, in the handle) peels the dependency graph in gated rounds through run_batches: wait[r] = the
// entries of r's list; round L settles its work list at level L and gives every dependant ONE atomic decrement per
// entry of the flipped lists ("who waits for me"); the one lane that reads the old value 1 owns the row and appends it
// to the next round's list.  A decrement is final (the word never rises), so the owner is unique: no compare-and-swap, no
// restore.  A row's wait reaches zero in the round after the last of its list settled: that is the definition of level.
// One sort of (level << bits | row) then gives order; the widths of the rounds give lstart on the host.
//
// THE SOLVE: x[r] = (b[r] - S_r) / d[r] (no division when unit), S_r = the sum of r's list with the terms
// t_j = (double)val_j * x[col_j], each product rounded once (no fused multiply-add).  THE SUM OF A LIST (trsv_list_sum)
// is sh_bc's shape: pieces of TRSV_PIECE entries, inside a piece 64 strided partials each started from +0.0, the fixed
// butterfly for o = 32, 16, 8, 4, 2, 1, the piece sums left to right from +0.0.  Terms are SIGNED here, so the one-lane
// tier of a list of at most TRSV_LANE entries computes +0.0 + t[k], not t[k]: a partial is never -0.0, padding with +0.0
// is then exact, and the three tiers (a lane, a wave, a wave over several pieces) are ONE function of the list.
//
// ONE OWNER PER VALUE.  x[r] is written by the one lane that owns row r of its level; what it reads was written by a
// launch that ended before (trsv_level) or by a level of the same launch that ended at a workgroup barrier before
// (trsv_run).  There is no float atomic.
//
// trsv_level is one ungated launch for a wide level.  trsv_run is one launch of ONE WORKGROUP for a run of consecutive
// thin levels with __syncthreads() between them: x is written and read inside the launch, by waves of one workgroup
// only, so it is NOT __restrict__, is read by plain loads (no read-only, no non-temporal path), and the barrier's
// release and acquire at workgroup scope order the stores of a level before the loads of the next.  No agent fence, no
// flag, no spin: NO KERNEL EVER WAITS for another kernel's write, and inside trsv_run a wave only waits at the barrier
// that all waves of its workgroup reach (the level loop's bounds are kernel arguments and lstart words: uniform).
// EVERY LOOP IS BOUNDED by a list length, a level's width, TRSV_RUN or `rows`.  Values are written with vector stores,
// atomics or plain C++ only.
//
// Worst cases.  A path (a bidiagonal matrix): `rows` levels of one row; the analysis pays two launches per level, the
// solve one barrier per level and one launch per TRSV_RUN levels.  A hub row: its list is summed by one wave alone, 64
// entries at a time.  A hub column: its dependants are decremented in pieces of TRSV_PIECE entries.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int TRSV_LANE = 8;              // lists up to this many entries: one lane each (the butterfly's last three levels)
constexpr int TRSV_PIECE = 2048;          // a piece of a list: 64 strided partials and one butterfly
constexpr int TRSV_BATCH = 32;            // rounds of the analysis enqueued ahead of the host at most (the first batch holds 8)
constexpr int TRSV_MAX_BLOCKS = 1024;     // workgroups of a launch at most: one WlPart each
constexpr int TRSV_CTL_BYTES = 1024;      // device bytes set aside for TrsvCtl
constexpr int TRSV_PART_BYTES = 16 * TRSV_MAX_BLOCKS;
// Levels of one trsv_run launch at most.  A level inside a run costs a barrier and a chain of dependent loads (order,
// ptr, col / val, x) and one store: a few microseconds, so 1024 levels keep a launch in the low milliseconds.
#ifndef SH_TRSV_RUN
#define SH_TRSV_RUN 1024
#endif
constexpr int TRSV_RUN = SH_TRSV_RUN;
constexpr int TRSV_THIN = 256;            // the default `thin`: a level of one row per thread of a workgroup at most
constexpr int TRSV_THIN_MAX = 1 << 16;    // the largest `thin`: a level of a run is walked by 256 lanes
static_assert(TRSV_LANE == 8, "trsv_list_sum writes the last three levels of the butterfly out for eight terms");
static_assert(TRSV_RUN >= 1, "a run holds a level");

struct TrsvRec {   // what round k of a batch of the analysis did (read back by the host once per batch)
  int32_t ran;
  uint32_t size, edges, pad;   // the rows of the level; the flipped-list entries walked
};
// Control block of the analysis in device memory.
struct TrsvCtl {
  int32_t step;                 // the round that runs next (-1 once the analysis has ended)
  int32_t finished;
  uint32_t n[2], np[2];         // length of work list 0 / 1, of its piece list
  int32_t p;                    // the list the next round walks
  uint32_t settled;
  TrsvRec rec[TRSV_BATCH];
};

struct TrsvFlip {   // the flipped lists and the analysis' state, as a kernel argument
  int32_t rows;
  const int32_t *out_ptr, *out_row;
  int32_t *wait, *level;
  uint32_t *list[2];
  WlPiece *pieces[2];
};
struct TrsvLists {   // the handle's lists as a kernel argument
  const int32_t *ptr, *col;
  const float *val;
  const double *d;
  const uint32_t *order;
};
struct TrsvIo {      // b: rows float32 (f32) or float64; x: rows float64 (the caller's, or the handle's own when f32); xf: the caller's float32 x
  const void *b;
  double *x;
  float *xf;
  int32_t f32, unit;
};

// ---- building the handle (once) -----------------------------------------------------------------------------------------
// flag[j] = entry j joins a list: its column is inside the matrix and strictly on the side of `uplo` (0: c < r, 1: c > r),
// whatever its value (flag[nnz] = 0 closes the scan)
__global__ __launch_bounds__(WL_BS) void trsv_flag(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx, int64_t nnz,
                                                    int32_t rows, int32_t uplo, uint32_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz) {
    const int32_t c = col_idx[j], r = wl_row_of(row_ptr, rows, j);
    flag[j] = ((uint32_t)c < (uint32_t)rows && (uplo ? c > r : c < r)) ? 1u : 0u;
  } else if (j == nnz) flag[j] = 0u;
}
// pos = exclusive scan of flag: survivor j -> key[pos[j]] = (r << bits | c), word[pos[j]] = its value's bits (in stored order)
__global__ __launch_bounds__(WL_BS) void trsv_keys(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                    const uint32_t *__restrict__ val, const uint32_t *__restrict__ flag,
                                                    const uint32_t *__restrict__ pos, int64_t nnz, int32_t rows, int bits,
                                                    uint64_t *__restrict__ key, uint32_t *__restrict__ word) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz && flag[j]) {
    key[pos[j]] = ((uint64_t)(uint32_t)wl_row_of(row_ptr, rows, j) << bits) | (uint64_t)(uint32_t)col_idx[j];
    word[pos[j]] = val[j];
  }
}
// d[r] = the diagonal entries of row r, widened and added left to right from +0.0 (one lane per row: one-off work);
// zero[0] += the rows with d == 0, zero[1] = the smallest of them (the host has set zero[] = {0, 0xFFFFFFFF})
__global__ __launch_bounds__(WL_BS) void trsv_diag(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                    const float *__restrict__ val, int32_t rows, double *__restrict__ d, uint32_t *zero) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  double sum = 0.0;
  if (r < rows)
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++)
      if ((int64_t)col_idx[j] == r) sum = sum + (double)val[j];
  const bool is_zero = r < rows && sum == 0.0;
  if (r < rows) d[r] = sum;
  const uint32_t n = wl_wave_sum(is_zero ? 1u : 0u), first = wl_wave_min(is_zero ? (uint32_t)r : 0xFFFFFFFFu);
  if (wl_lane() == 0 && n) {
    wl_add(&zero[0], n);
    (void)wl_umin(&zero[1], first);
  }
}
// The flipped key of every sorted key: okey[i] = (c << bits | r), to be sorted ("who waits for me")
__global__ __launch_bounds__(WL_BS) void trsv_flip(const uint64_t *__restrict__ key, int64_t n, int bits, uint64_t *__restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n) okey[i] = ((key[i] & ((1ull << bits) - 1ull)) << bits) | (key[i] >> bits);
}

// ---- the analysis ---------------------------------------------------------------------------------------------------------
// wait[r] = the entries of r's list; the rows that wait for nobody are round 0's work list (the host has zeroed the
// control block: step 0, list 0)
__global__ __launch_bounds__(WL_BS) void trsv_seed(TrsvCtl *ctl, const int32_t *__restrict__ ptr, TrsvFlip F) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < F.rows; base += wl_waves() * 64) {
    const int64_t r = base + lane;
    const int32_t len = r < F.rows ? ptr[r + 1] - ptr[r] : 1;
    if (r < F.rows) { F.wait[r] = len; F.level[r] = 0; }
    const uint32_t at = wl_wave_append(&ctl->n[0], len == 0, lane);
    if (len == 0) {
      F.list[0][at] = (uint32_t)r;
      wl_push_pieces<TRSV_PIECE>(&ctl->np[0], (uint32_t)r, (uint32_t)(F.out_ptr[r + 1] - F.out_ptr[r]), F.pieces[0]);
    }
  }
}
// Round L: the rows of the work list are level L; every dependant gets one decrement per entry, and the lane that takes
// the last one owns it.
__global__ __launch_bounds__(WL_BS) void trsv_settle(TrsvCtl *ctl, int L, TrsvFlip F, WlPart *__restrict__ part) {
  if (ctl->step != L) return;
  const int p = ctl->p, q = p ^ 1;
  const uint32_t looked = wl_expand<TRSV_LANE, TRSV_PIECE>(
      F.list[p], (int64_t)ctl->n[p], F.pieces[p], (int64_t)ctl->np[p], F.out_ptr,
      [&](int32_t v, bool first) { if (first) F.level[v] = L; return 0u; },
      [&](int32_t j, uint32_t) {
        const int32_t u = F.out_row[j];
        if (__hip_atomic_fetch_add(&F.wait[u], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 1) return;
        F.list[q][wl_append_here(&ctl->n[q])] = (uint32_t)u;
        wl_push_pieces<TRSV_PIECE>(&ctl->np[q], (uint32_t)u, (uint32_t)(F.out_ptr[u + 1] - F.out_ptr[u]), F.pieces[q]);
      });
  wl_block_part(part, looked, 0u);
}
// Closes round L (slot k of the batch).  One workgroup folds the WlParts and its first thread records the round and decides.
__global__ __launch_bounds__(WL_BS) void trsv_close(TrsvCtl *ctl, int k, int L, int nparts, const WlPart *__restrict__ part) {
  if (!wl_from_thread0(ctl->step == L)) return;
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x != 0) return;
  const int p = ctl->p;
  ctl->rec[k] = TrsvRec{1, ctl->n[p], sums.a, 0u};
  ctl->settled += ctl->n[p];
  ctl->n[p] = 0u; ctl->np[p] = 0u;
  ctl->p = p ^ 1;
  if (ctl->n[p ^ 1] == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = L + 1;
}
// key[r] = (level << bits | r), to be sorted; and back: order[i] = the row of sorted key i
__global__ __launch_bounds__(WL_BS) void trsv_rank_keys(const int32_t *__restrict__ level, int32_t rows, int bits, uint64_t *__restrict__ key) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (r < rows) key[r] = ((uint64_t)(uint32_t)level[r] << bits) | (uint64_t)r;
}
__global__ __launch_bounds__(WL_BS) void trsv_order(const uint64_t *__restrict__ key, int32_t rows, int bits, uint32_t *__restrict__ order) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < rows) order[i] = (uint32_t)(key[i] & ((1ull << bits) - 1ull));
}

// ---- the sum of a list ----------------------------------------------------------------------------------------------------
// The butterfly over the wave's 64 partials -> every lane (wave-uniform control flow only).  Its order is part of the
// result: it is written out here and restated by tests/trsv_ref.py and host/src/trsv_solve.cpp.
__device__ __forceinline__ double trsv_butterfly(double v) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}
// Every lane of the wave brings a list (s, len; `valid`); term(j) is the term of entry j.  -> for the lane that brought
// the list, its sum as the header defines it.  (Wave-uniform control flow only: the whole wave calls it together.)
// The gathers of four of a lane's entries, or of TRSV_FLIGHT strides of a piece, are issued together: an entry behind
// the list's end reads the list's last entry instead (a valid address) and its term is replaced by +0.0, which a
// partial that is never -0.0 absorbs exactly; the additions stay in the order of the definition (DESIGN.md 6q has the
// measurements of the three forms that were tried).
constexpr int TRSV_FLIGHT = 4;   // strides of a piece whose gathers are in flight together
template <class Term>
__device__ __forceinline__ double trsv_list_sum(bool valid, int32_t s, int32_t len, Term term) {
  const int lane = wl_lane();
  double sum = 0.0;
  if (!valid) len = 0;
  if (len > 0 && len <= TRSV_LANE) {   // partial[l] = +0.0 + t[l] (never -0.0), and the butterfly's levels 32, 16 and 8 add +0.0
    double t[TRSV_LANE];
#pragma unroll
    for (int k = 0; k < TRSV_LANE / 2; k++) t[k] = term(s + min(k, len - 1));
#pragma unroll
    for (int k = TRSV_LANE / 2; k < TRSV_LANE; k++) t[k] = 0.0;
    if (len > TRSV_LANE / 2) {   // (most lists of a factor are short: the second four gathers only where there are entries for them)
#pragma unroll
      for (int k = TRSV_LANE / 2; k < TRSV_LANE; k++) t[k] = term(s + min(k, len - 1));
    }
#pragma unroll
    for (int k = 0; k < TRSV_LANE; k++) t[k] = k < len ? 0.0 + t[k] : 0.0;
    sum = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
  }
  uint64_t m = __ballot(len > TRSV_LANE);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
    double acc = 0.0;
    for (int32_t p0 = 0; p0 < lb; p0 += TRSV_PIECE) {   // the pieces, left to right
      const int32_t pe = min(lb, p0 + TRSV_PIECE);
      double partial = 0.0;
      for (int32_t j = p0 + lane; j < pe; j += 64 * TRSV_FLIGHT) {
        double t[TRSV_FLIGHT];
#pragma unroll
        for (int u = 0; u < TRSV_FLIGHT; u++) t[u] = term(sb + min(j + 64 * u, pe - 1));
#pragma unroll
        for (int u = 0; u < TRSV_FLIGHT; u++) partial = partial + (j + 64 * u < pe ? t[u] : 0.0);
      }
      acc = acc + trsv_butterfly(partial);
    }
    if (lane == src) sum = acc;
  }
  return sum;
}

// ---- the solve --------------------------------------------------------------------------------------------------------------
// The rows order[a, b), one lane each, 64 per wave: wave `first` of `stride` waves.  x of the lists' columns was written
// before this level began (by an earlier launch or before the barrier): plain loads.
__device__ __forceinline__ void trsv_rows(int64_t a, int64_t b, int64_t first, int64_t stride, const TrsvLists &T, const TrsvIo &Io) {
  const int lane = wl_lane();
  for (int64_t base = a + first * 64; base < b; base += stride * 64) {
    const bool valid = base + lane < b;
    const int32_t r = valid ? (int32_t)T.order[base + lane] : 0;
    const int32_t s = valid ? T.ptr[r] : 0;
    const int32_t len = valid ? T.ptr[r + 1] - s : 0;
    const double sum = trsv_list_sum(valid, s, len, [&](int32_t j) { return (double)T.val[j] * Io.x[T.col[j]]; });
    if (valid) {
      const double rhs = Io.f32 ? (double)((const float *)Io.b)[r] : ((const double *)Io.b)[r];
      double v = rhs - sum;
      if (!Io.unit) v = v / T.d[r];
      Io.x[r] = v;
      if (Io.f32) Io.xf[r] = (float)v;
    }
  }
}
// A wide level order[a, b): ungated, the grid sized by its width (the host knows lstart), capped, with a grid-stride loop.
__global__ __launch_bounds__(WL_BS) void trsv_level(uint32_t a, uint32_t b, TrsvLists T, TrsvIo Io) {
  trsv_rows((int64_t)a, (int64_t)b, wl_wave(), wl_waves(), T, Io);
}
// The thin levels L0 ... L0 + n - 1 (n <= TRSV_RUN) in ONE workgroup (the grid is 1), a workgroup barrier between them.
__global__ __launch_bounds__(WL_BS) void trsv_run(int32_t L0, int32_t n, const uint32_t *__restrict__ lstart, TrsvLists T, TrsvIo Io) {
  for (int32_t L = L0; L < L0 + n; L++) {
    trsv_rows((int64_t)lstart[L], (int64_t)lstart[L + 1], (int64_t)(threadIdx.x >> 6), WL_BS / 64, T, Io);
    __syncthreads();   // (release and acquire at workgroup scope: the level's x before the next level's loads)
  }
}

} // namespace sh
