// ilu0.hip.h -- kernels of sh_ilu0: the incomplete LU factorisation without fill, ILU(0) (Meijerink, van der Vorst,
// Math. Comp. 1977; Saad, "Iterative Methods for Sparse Linear Systems", 2nd ed., algorithm 10.4, the row-wise IKJ
// form), BY LEVEL SETS (Naumov, "Parallel incomplete-LU and Cholesky factorization in the preconditioned iterative
// methods on the GPU", NVIDIA NVR-2012-003), in float64 and in ONE FIXED ORDER, so that the factor is a function of the
// pattern and the values alone and is compared with == (DESIGN.md "6r Incomplete LU factorisation").
//
// THE SLOTS.  The handle is made from the pattern alone.  The entries with a column inside the matrix become 64-bit keys
// (r << bits | c) with their position riding along, sorted by one stable radix sort; the first key of every run of equal
// keys is a SLOT: ptr / col hold the slots of every row in ascending column, gstart / perm the entries of every slot in
// the order given, slot_of[p] / head[p] the slot and the headship of input position p (slot_of = -1 outside the
// matrix).  dslot[r] = the diagonal slot of row r or -1; up[r] = the first slot of r right of the diagonal;
// rwork[r] = the look-ups of row r's elimination (the sum over its lower slots (r, k) of the upper slots of row k,
// capped at 2^31 - 1).  w = one float64 per slot: the working array of a call.
//
// THE LEVELS are sh_trsv's of the lower triangle (uplo = 0): the engine runs that analysis (trsv.hip.h, gated rounds of
// atomic decrements, no compare-and-swap) and this handle keeps level, order and lstart.  Row r reads rows k < r of
// lower levels only, and writes its own slots only.
//
// A CALL.  ilu0_load: w[s] = the entries of slot s widened and added left to right from +0.0.  Then sh_trsv's plan: one
// ungated launch per wide level (ilu0_level), one launch of ONE WORKGROUP per run of consecutive thin levels (ilu0_run)
// with a workgroup barrier between levels.  ilu0_store: lu[p] = w[slot_of[p]] for a head, +0.0 for every other
// position, and the zero pivots counted by wave sums, one atomic per wave.
//
// THE ELIMINATION OF A ROW (ilu0_step, ilu0_update: ONE sequence of operations per slot, whichever tier runs it).  For
// every lower slot s = (r, k) in ascending k: wk = w[s] / u[k, k] (the final value of row k's diagonal slot; +0.0 where
// there is none), w[s] = wk, and for every upper slot t = (k, j) of row k in ascending j, the slot q = (r, j), found by
// bisection of row r's columns right of s, gets w[q] = w[q] - wk * w[t]: the product rounded once, the subtraction a
// second rounding (-ffp-contract=off).  A slot q so receives its subtractions in ascending k, one after the other.
//   The LANE tier: a row with rwork <= ILU0_LANE_WORK is eliminated by its lane alone, in program order.
//   The WAVE tier: the others are taken one at a time by the whole wave (a ballot loop, as trsv_list_sum's); inside a
//   step k the lanes stride over the upper slots of row k; distinct j of one row k are distinct slots of r, so no two
//   lanes write one word, and no lane reads a word of row r that a step writes (it reads w[s], w[t] of row k and its own
//   w[q]).  Between steps the wave meets at wl_wave_sync().
//
// ONE OWNER PER VALUE.  Every w[q] of row r is written by the wave that owns r in its level; inside a step by one lane.
// There is no float atomic.
//
// WHY THE IN-LAUNCH FORMS ARE SOUND.  w is written and re-read inside one launch, so it is NOT __restrict__ and is read
// by plain loads only (no read-only path, no non-temporal path).  (1) Between the levels of ilu0_run: the waves of ONE
// workgroup, and __syncthreads() is a release and an acquire at workgroup scope: the stores of a level come before the
// loads of the next -- trsv_run's argument.  (2) Between the steps of the wave tier: lane a's store to w[q] in step k may
// be lane b's load of w[q] (the next step's w[s], or the same q under another j' -- never in the same step) in step k'.
// Both are vector memory instructions of ONE wave: they are issued in program order to one vector L1, which keeps the
// accesses of a wave to one address in order, so the hardware needs nothing (the AMDGPU memory model asks for no code
// at wavefront scope); what is needed is that the COMPILER neither moves the load above the store nor keeps an earlier
// value in a register.  wl_wave_sync() is that: a release fence at wavefront scope, the wave barrier, an acquire fence
// at wavefront scope.  It is reached in wave-uniform control flow (the step loop's bounds are broadcast values).  No
// agent fence, no flag, no spin: NO KERNEL EVER WAITS for another kernel's write.  (3) Between launches: stream order.
// EVERY LOOP IS BOUNDED by a row's length, its logarithm, a level's width, ILU0_RUN or `rows`.  Values are written with
// vector stores, atomics or plain C++ only.
//
// Worst cases.  A dense hub row against long rows k: one wave does all of rwork[r] look-ups, 64 at a time (a workgroup
// tier is not built).  A path (a tridiagonal matrix): `rows` levels of one row, one barrier per level and one launch per
// ILU0_RUN levels; a host loop wins.
#pragma once
#include "worklist.hip.h"

namespace sh {

// A row whose elimination takes at most this many look-ups (rwork) is its lane's alone; above it the whole wave takes
// the row.  THE DEFAULT IS THE SWEEP'S: of 16, 64, 256, 1024 and 4096 (tools/ilu0_bench.py) 256 was the
// fastest on synth:scircuit and on R-MAT-14, 16 to 256 lying within 4 % of one another, and the 2048^2 grid is
// indifferent (its rows have four look-ups); -DSH_ILU0_LANE_WORK=n overrides it for such a sweep.
#ifndef SH_ILU0_LANE_WORK
#define SH_ILU0_LANE_WORK 256
#endif
constexpr int ILU0_LANE_WORK = SH_ILU0_LANE_WORK;
// Levels of one ilu0_run launch at most (SH_TRSV_RUN's reasoning: a level in a run costs a barrier and a chain of
// dependent loads).
#ifndef SH_ILU0_RUN
#define SH_ILU0_RUN 1024
#endif
constexpr int ILU0_RUN = SH_ILU0_RUN;
constexpr int ILU0_THIN = 256;            // the default `thin`: a level of one row per thread of a workgroup at most
constexpr int ILU0_THIN_MAX = 1 << 16;    // the largest `thin`
constexpr int ILU0_MAX_BLOCKS = 1024;     // workgroups of a launch at most
constexpr int ILU0_FIG_BYTES = 16;        // the figures of a call: zero pivots, the first of them; of the build: work
static_assert(ILU0_LANE_WORK >= 0 && ILU0_RUN >= 1, "a run holds a level");

struct Ilu0Lists {   // the handle as a kernel argument (w is written and re-read inside a launch: no member is restrict)
  const int32_t *ptr, *col, *dslot, *up, *rwork;
  const uint32_t *order;
  double *w;
};

// ---- building the handle (once) -----------------------------------------------------------------------------------------
// flag[j] = entry j has a column inside the matrix (flag[nnz] = 0 closes the scan)
__global__ __launch_bounds__(WL_BS) void ilu0_flag(const int32_t *__restrict__ col_idx, int64_t nnz, int32_t rows, uint32_t *__restrict__ flag) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz) flag[j] = (uint32_t)col_idx[j] < (uint32_t)rows ? 1u : 0u;
  else if (j == nnz) flag[j] = 0u;
}
// pos = exclusive scan of flag: survivor j -> key[pos[j]] = (r << bits | c), word[pos[j]] = j (in stored order)
__global__ __launch_bounds__(WL_BS) void ilu0_keys(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                    const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int64_t nnz,
                                                    int32_t rows, int bits, uint64_t *__restrict__ key, uint32_t *__restrict__ word) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j < nnz && flag[j]) {
    key[pos[j]] = ((uint64_t)(uint32_t)wl_row_of(row_ptr, rows, j) << bits) | (uint64_t)(uint32_t)col_idx[j];
    word[pos[j]] = (uint32_t)j;
  }
}
// Sorted key i (of n; head = wl_run_heads, hpos = its exclusive scan, perm = the positions that rode along): its slot
// is hpos[i] for a head and hpos[i] - 1 behind one.  slot_of / head by input position (the host has set slot_of = -1,
// head = 0); a head gives its slot's key and first entry; gstart[slots] = n closes the groups.
__global__ __launch_bounds__(WL_BS) void ilu0_slots(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                     const uint32_t *__restrict__ hpos, const uint32_t *__restrict__ perm, int64_t n,
                                                     int32_t *__restrict__ slot_of, uint32_t *__restrict__ head_of,
                                                     uint64_t *__restrict__ ukey, int32_t *__restrict__ gstart) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n) {
    const uint32_t h = head[i], s = hpos[i] - (h ? 0u : 1u);
    slot_of[perm[i]] = (int32_t)s;
    head_of[perm[i]] = h;
    if (h) { ukey[s] = key[i]; gstart[s] = (int32_t)i; }
  } else if (i == n) gstart[hpos[n]] = (int32_t)n;
}
// dslot[r] = the diagonal slot of row r or -1, up[r] = its first slot right of the diagonal (one lane per row, a
// bisection of its sorted columns); fig[0] += the rows without a diagonal slot, fig[1] = the smallest of them (the
// host has set fig[] = {0, 0xFFFFFFFF})
__global__ __launch_bounds__(WL_BS) void ilu0_diag(const int32_t *__restrict__ ptr, const int32_t *__restrict__ col, int32_t rows,
                                                    int32_t *__restrict__ dslot, int32_t *__restrict__ up, uint32_t *fig) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  bool missing = false;
  if (r < rows) {
    int32_t lo = ptr[r], hi = ptr[r + 1];   // the first slot with a column >= r
    const int32_t end = hi;
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (col[mid] < (int32_t)r) lo = mid + 1; else hi = mid;
    }
    missing = !(lo < end && col[lo] == (int32_t)r);
    dslot[r] = missing ? -1 : lo;
    up[r] = missing ? lo : lo + 1;
  }
  const uint32_t n = wl_wave_sum(missing ? 1u : 0u), first = wl_wave_min(missing ? (uint32_t)r : 0xFFFFFFFFu);
  if (wl_lane() == 0 && n) {
    wl_add(&fig[0], n);
    (void)wl_umin(&fig[1], first);
  }
}
// rwork[r] = the sum over the lower slots (r, k) of the upper slots of row k, capped at 2^31 - 1 (one lane per row:
// one-off work); *work += the uncapped sums (one 64-bit integer atomic per lane with work: one-off too)
__global__ __launch_bounds__(WL_BS) void ilu0_work(const int32_t *__restrict__ ptr, const int32_t *__restrict__ col,
                                                    const int32_t *__restrict__ up, int32_t rows, int32_t *__restrict__ rwork,
                                                    unsigned long long *work) {
  const int64_t r = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (r >= rows) return;
  unsigned long long sum = 0;
  for (int32_t s = ptr[r]; s < ptr[r + 1] && col[s] < (int32_t)r; s++) {
    const int32_t k = col[s];
    sum += (unsigned long long)(ptr[k + 1] - up[k]);
  }
  rwork[r] = (int32_t)(sum < 0x7FFFFFFFull ? sum : 0x7FFFFFFFull);
  if (sum) (void)__hip_atomic_fetch_add(work, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- a call ---------------------------------------------------------------------------------------------------------------
// w[s] = the entries of slot s in the order given, widened and added left to right from +0.0
__global__ __launch_bounds__(WL_BS) void ilu0_load(const int32_t *__restrict__ gstart, const uint32_t *__restrict__ perm,
                                                    const float *__restrict__ val, int64_t slots, double *__restrict__ w) {
  const int64_t s = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (s >= slots) return;
  double sum = 0.0;
  for (int32_t i = gstart[s]; i < gstart[s + 1]; i++) sum = sum + (double)val[perm[i]];
  w[s] = sum;
}

// Step t = (k, j) of the elimination of a row whose slots right of the step's lower slot are [lo, end): the slot
// q = (r, j), if there is one, loses wk * u[k, j].
__device__ __forceinline__ void ilu0_update(const Ilu0Lists &T, int32_t t, int32_t lo, int32_t end, double wk) {
  const int32_t j = T.col[t];
  int32_t hi = end;
  while (lo < hi) {   // the first slot of [lo, end) with a column >= j
    const int32_t mid = lo + (hi - lo) / 2;
    if (T.col[mid] < j) lo = mid + 1; else hi = mid;
  }
  if (lo < end && T.col[lo] == j) {
    const double p = wk * T.w[t];
    T.w[lo] = T.w[lo] - p;
  }
}
// The multiplier of the lower slot s = (r, k): w[s] / u[k, k], a missing diagonal slot being +0.0
__device__ __forceinline__ double ilu0_step(const Ilu0Lists &T, int32_t s, int32_t k) {
  const int32_t dk = T.dslot[k];
  const double piv = dk >= 0 ? T.w[dk] : 0.0;
  return T.w[s] / piv;
}
// The rows order[a, b), 64 per wave: wave `first` of `stride` waves.  The rows k they read were finished before this
// level began (by an earlier launch or before the barrier).
__device__ __forceinline__ void ilu0_rows(int64_t a, int64_t b, int64_t first, int64_t stride, const Ilu0Lists &T) {
  const int lane = wl_lane();
  for (int64_t base = a + first * 64; base < b; base += stride * 64) {
    const bool valid = base + lane < b;
    const int32_t r = valid ? (int32_t)T.order[base + lane] : 0;
    const int32_t s0 = valid ? T.ptr[r] : 0, end = valid ? T.ptr[r + 1] : 0;
    const int32_t d = valid ? T.dslot[r] : 0;
    const int32_t lend = valid ? (d >= 0 ? d : T.up[r]) : 0;   // the lower slots are [s0, lend)
    const bool wide = valid && T.rwork[r] > ILU0_LANE_WORK;
    if (!wide) {   // the lane tier (a lane without a row has no lower slot)
      for (int32_t s = s0; s < lend; s++) {
        const int32_t k = T.col[s];
        const double wk = ilu0_step(T, s, k);
        T.w[s] = wk;
        for (int32_t t = T.up[k]; t < T.ptr[k + 1]; t++) ilu0_update(T, t, s + 1, end, wk);
      }
    }
    uint64_t m = __ballot(wide);
    if (m) wl_wave_sync();   // (the lane tier's stores are other rows': nothing to order, but the loop below starts clean)
    while (m) {              // the wave tier: one row at a time, every bound a broadcast value
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s0, src), eb = __shfl(end, src), lb = __shfl(lend, src);
      for (int32_t s = sb; s < lb; s++) {
        const int32_t k = T.col[s];
        const double wk = ilu0_step(T, s, k);
        if (lane == 0) T.w[s] = wk;
        const int32_t te = T.ptr[k + 1];
        for (int32_t t = T.up[k] + lane; t < te; t += 64) ilu0_update(T, t, s + 1, eb, wk);
        wl_wave_sync();   // this step's stores before the next step's loads
      }
    }
  }
}
// A wide level order[a, b): ungated, the grid sized by its width (the host knows lstart), capped, with a grid-stride loop.
__global__ __launch_bounds__(WL_BS) void ilu0_level(uint32_t a, uint32_t b, Ilu0Lists T) {
  ilu0_rows((int64_t)a, (int64_t)b, wl_wave(), wl_waves(), T);
}
// The thin levels L0 ... L0 + n - 1 (n <= ILU0_RUN) in ONE workgroup (the grid is 1), a workgroup barrier between them.
__global__ __launch_bounds__(WL_BS) void ilu0_run(int32_t L0, int32_t n, const uint32_t *__restrict__ lstart, Ilu0Lists T) {
  for (int32_t L = L0; L < L0 + n; L++) {
    ilu0_rows((int64_t)lstart[L], (int64_t)lstart[L + 1], (int64_t)(threadIdx.x >> 6), WL_BS / 64, T);
    __syncthreads();   // (release and acquire at workgroup scope: the level's w before the next level's loads)
  }
}
// lu[p] = the slot's value for the first entry of its group, +0.0 for a later one or a column outside the matrix
// (float32, rounded once, when f32; else float64); thread r < rows also looks at row r's pivot: fig[0] += the rows whose
// pivot == 0.0 (a missing diagonal slot is +0.0; a NaN does not count), fig[1] = the smallest of them (the host has set
// fig[] = {0, 0xFFFFFFFF}).  The grid covers max(nnz, rows).
__global__ __launch_bounds__(WL_BS) void ilu0_store(const int32_t *__restrict__ slot_of, const uint32_t *__restrict__ head_of,
                                                     const int32_t *__restrict__ dslot, const double *__restrict__ w, int64_t nnz,
                                                     int32_t rows, int32_t f32, void *__restrict__ lu, uint32_t *fig) {
  const int64_t p = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (p < nnz) {
    const double v = head_of[p] ? w[slot_of[p]] : 0.0;
    if (f32) ((float *)lu)[p] = (float)v; else ((double *)lu)[p] = v;
  }
  bool is_zero = false;
  if (p < rows) {
    const int32_t d = dslot[p];
    is_zero = (d >= 0 ? w[d] : 0.0) == 0.0;
  }
  const uint32_t n = wl_wave_sum(is_zero ? 1u : 0u), first = wl_wave_min(is_zero ? (uint32_t)p : 0xFFFFFFFFu);
  if (wl_lane() == 0 && n) {
    wl_add(&fig[0], n);
    (void)wl_umin(&fig[1], first);
  }
}

} // namespace sh
