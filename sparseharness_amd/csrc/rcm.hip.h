// rcm.hip.h -- kernels of sh_rcm: the reverse Cuthill-McKee ordering of the simple undirected graph under a square matrix
// (Cuthill, McKee, "Reducing the bandwidth of sparse symmetric matrices", ACM 1969; the reversal: George 1971; the root
// by George, Liu, "An implementation of a pseudoperipheral node finder", ACM TOMS 1979, with a cap on the sweeps), in
// level-synchronous steps (DESIGN.md "6o Reverse Cuthill-McKee").
//
// LABEL SPACE.  The handle sorts the vertices once by (deg, index) and keeps S[label] = vertex; the symmetric lists
// ptr[rows + 1] / col[2M] are built over the labels, every list strictly ascending.  So "the smaller (deg, index)" is
// the smaller label, every list already stands in child order, "the smallest vertex of the last level" is a 32-bit
// atomic minimum and "the next unnumbered vertex of the walk" a cursor over the labels.  Labels 0 .. zeros - 1 are the
// vertices without an edge; rcm_init settles them.  Only rcm_finish maps back through S.
//
// The state of a call: order[k] = the label at (un-reversed) position k, posl[l] = the position of label l or -1,
// levl[l] = its level from its component's final root or -1, stamp[l] = the generation of the last sweep that reached l
// (generations count DOWN from 0xFFFFFFFE, so claiming is an atomic minimum and nothing is cleared between sweeps),
// owner[l] = the smallest position that claimed l (0xFFFFFFFF before), cnt[i] = the children of position i.
// `done` = the positions given so far.  order[done, rows) is free while a component is swept, and a sweep uses it as
// its queue: a component holds at most rows - done vertices.
//
// A STEP is one level of one breadth-first search, and a fixed set of five launches, each of which returns at once
// unless the control block says the step is its turn and of its kind:
//   kind 0, a sweep level (unordered): rcm_sweep walks the lists of the level order[a, b); an entry whose stamp is not
//       the sweep's generation is claimed by the one lane whose atomic minimum reads an older stamp, is appended at the
//       atomic cursor `tail` and folds its label into `xmin`.
//   kind 1, a numbering level: rcm_claim: atomicMin(owner[w], i) for every unnumbered entry w of the list of position i
//       in [a, b).  rcm_count: cnt[i] = the entries of i's list with owner == i; a workgroup takes a contiguous chunk of
//       positions and leaves its total in a WlPart.  rcm_place: every workgroup adds up the totals before its own, scans
//       its chunk, and position i writes its children at b + offset(i) + k in list order with posl and levl.
//   rcm_close, one workgroup: records the step and chooses the next one: the next level, a sweep from x, the numbering
//       from r, the next component (the cursor advances to the next label with posl < 0), or the end.
// A position is given once per call, so owner[w] == i can hold for the one level in which i is walked only: rcm_count
// and rcm_place need no other test, and neither reads a word that its launch writes.
//
// THE LEVEL FORM IS THE SERIAL FORM.  The serial loop takes the vertices in position order and appends each one's
// unnumbered neighbours in ascending label.  A vertex w of the next level is appended by the first position that has it
// in its list, i.e. the smallest position i of [a, b) adjacent to w: owner[w].  So the next level is the concatenation,
// over i ascending, of the entries of i's list owned by i, in list order; and every vertex of the level after that has
// no neighbour before a.  The order array is its own queue and nothing is sorted.
//
// The list walk (rcm_tile) has three tiers, and all of them give an entry its rank among the chosen entries of its list:
//   a lane       lists of up to RCM_LANE = 8 entries;
//   a wave       up to RCM_WAVE = 2048 entries, 64 at a time, ranked by a ballot prefix;
//   a workgroup  longer ones, WL_BS = 256 at a time, ranked by a ballot prefix and the four waves' counts.
//
// Invariant 1: EVERY VERTEX GETS ONE POSITION.  owner[w] is written for unnumbered w only and by atomic minimum, so after
// rcm_claim it names exactly one position of the level; the counts of rcm_count add up to the distinct vertices of the
// next level, and rcm_place writes order[b, b + total) once each: no place beyond rows - 1 is written.  A sweep appends
// a vertex once per generation: its queue stays inside order[done, rows).
// Invariant 2: NO KERNEL EVER WAITS for another kernel's write, and no lane for another lane's.  Every exchange between
// workgroups crosses a launch boundary.  There is no spin loop, no flag, no retry and no compare-and-swap: atomicMin,
// atomicAdd and stamps only.  The gate words (step, kind, a, b, gen, lvl) are written by rcm_close or rcm_begin alone;
// what a walking launch writes to the control block (tail, xmin) no workgroup of it reads.  Values are written with
// vector stores, atomics or plain C++ only.  max_steps bounds the call.
// Invariant 3: EVERY LOOP IS BOUNDED by a list length, a level's width, `rows` or the workgroups of a launch.
//
// Worst cases.  A step costs its five launches however narrow its level is: a path of n vertices takes about
// (sweeps' BFSs + 1) * n steps, the 2048 x 2048 grid 4095 per BFS.  A component of c vertices costs at least
// 2 (sweeps = 0) or 6 steps, so thousands of small components pay for each.  The cursor's scan is one workgroup's.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int RCM_LANE = 8;               // lists up to this many entries: one lane each
constexpr int RCM_WAVE = 2048;            // lists up to this: one wave; above: the workgroup
constexpr int RCM_BATCH = 32;             // steps enqueued ahead of the host at most (the first batch holds 8)
constexpr int RCM_MAX_BLOCKS = 1024;      // workgroups of a launch at most: one WlPart and one RcmFin each
constexpr int RCM_CTL_BYTES = 1024;       // device bytes set aside for RcmCtl
constexpr int RCM_PART_BYTES = 16 * RCM_MAX_BLOCKS;
constexpr int RCM_FIN_BYTES = 32 * RCM_MAX_BLOCKS;
constexpr int RCM_MAX_SWEEPS = 64;
constexpr uint32_t RCM_NONE = 0xFFFFFFFFu;

struct RcmRec {   // what step k of a batch did (read back by the host once per batch)
  int32_t ran, kind;
  uint32_t size, edges;   // the level's width, the sum of its list lengths
};
// Control block in device memory.
struct RcmCtl {
  int32_t step;                  // the step that runs next (-1 once the run has finished)
  int32_t finished;
  int32_t kind;                  // 0: a sweep level, 1: a numbering level
  int32_t sweeps, left;          // the call's cap, and the sweeps the component may still start
  uint32_t a, b;                 // the level: order[a, b)
  uint32_t tail;                 // kind 0: where the next level ends so far (atomic cursor)
  uint32_t xmin, xlast;          // the smallest label appended in this step; the smallest label of the level [a, b)
  uint32_t done, cursor;         // positions given; the label the walk stands at
  uint32_t gen;                  // the generation of the sweep that runs (counts down)
  int32_t lvl;                   // the level number of [a, b)
  uint32_t root, src;            // r; the source of the sweep that runs
  int32_t ecc;                   // e, the eccentricity of r (-1 until the first sweep of the component has ended)
  int32_t components, sweeps_run;
  uint32_t pad;
  int64_t bw[2], prof[2];        // bandwidth and profile: [0] under the identity, [1] under the new order (rcm_total)
  RcmRec rec[RCM_BATCH];
};
// The WlPart of a workgroup: a = the children it counted (rcm_count), b = list entries looked at (rcm_sweep, rcm_count).
struct RcmFin { uint32_t bw[2]; uint64_t prof[2]; uint64_t pad; };   // a workgroup's share of rcm_finish

struct RcmGraph {   // the handle's lists over the labels, as a kernel argument
  int32_t rows;
  const int32_t *ptr, *col;
};
struct RcmState {   // `rows` words each
  uint32_t *order;
  int32_t *posl, *levl;
  uint32_t *stamp, *owner, *cnt;
};

// ---- building the handle (once) -----------------------------------------------------------------------------------------
// key[v] = deg[v] << 32 | v: sorted ascending, position l holds the vertex of label l
__global__ __launch_bounds__(WL_BS) void rcm_vertex_keys(const uint32_t *__restrict__ deg, int64_t rows, uint64_t *__restrict__ key) {
  const int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (v < rows) key[v] = ((uint64_t)deg[v] << 32) | (uint64_t)v;
}
// S[l] = the vertex of label l, inv[S[l]] = l, *zeros = the labels without an edge (*zeros zeroed by the host; the one
// label that ends the run of degree 0 writes it)
__global__ __launch_bounds__(WL_BS) void rcm_labels(const uint64_t *__restrict__ sorted, int64_t rows, int32_t *__restrict__ S,
                                                     uint32_t *__restrict__ inv, uint32_t *__restrict__ zeros) {
  const int64_t l = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (l >= rows) return;
  const uint32_t v = (uint32_t)(sorted[l] & 0xFFFFFFFFull);
  S[l] = (int32_t)v;
  inv[v] = (uint32_t)l;
  if ((sorted[l] >> 32) == 0 && (l + 1 == rows || (sorted[l + 1] >> 32) != 0)) *zeros = (uint32_t)(l + 1);
}
// wl_both_ways over the labels: edge i of the simple graph (pos = exclusive scan of head) as
// okey[2 * pos[i]] = (inv[u] << bits | inv[v]) and okey[2 * pos[i] + 1] = (inv[v] << bits | inv[u])
__global__ __launch_bounds__(WL_BS) void rcm_both_ways(const uint64_t *__restrict__ key, const uint32_t *__restrict__ head,
                                                        const uint32_t *__restrict__ pos, int64_t n, int bits,
                                                        const uint32_t *__restrict__ inv, uint64_t *__restrict__ okey) {
  const int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (i < n && head[i]) {
    const uint64_t u = inv[key[i] >> bits], v = inv[key[i] & ((1ull << bits) - 1ull)];
    okey[2 * (int64_t)pos[i]] = (u << bits) | v;
    okey[2 * (int64_t)pos[i] + 1] = (v << bits) | u;
  }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------
// One tile: thread t of the workgroup brings a list (s, len; `valid`) with two carried words, key and base.  Every entry
// w of the list is asked pred(key, w) ONCE, and every chosen entry gets emit(key, base, w, rank), rank = the chosen
// entries of its list before it.  -> for the thread that brought the list, the chosen entries of it.
// (Convergent control flow only: the whole workgroup calls it together.)
template <class Pred, class Emit>
__device__ __forceinline__ uint32_t rcm_tile(const int32_t *__restrict__ col, bool valid, uint32_t key, uint32_t base, int32_t s, int32_t len,
                                             Pred pred, Emit emit) {
  __shared__ uint32_t s_nlong, s_long[WL_BS], s_bring[4], s_wcnt[WL_BS / 64];
  const int lane = wl_lane(), wv = (int)(threadIdx.x >> 6);
  const uint64_t below = (1ull << lane) - 1ull;
  uint32_t c = 0;
  if (!valid) len = 0;
  if (threadIdx.x == 0) s_nlong = 0u;
  if (len <= RCM_LANE)
    for (int32_t j = 0; j < len; j++) {
      const uint32_t w = (uint32_t)col[s + j];
      if (pred(key, w)) { emit(key, base, w, c); c++; }
    }
  uint64_t m = __ballot(len > RCM_LANE && len <= RCM_WAVE);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
    const uint32_t kb = (uint32_t)__shfl((int)key, src), bb = (uint32_t)__shfl((int)base, src);
    uint32_t run = 0;
    for (int32_t j0 = 0; j0 < lb; j0 += 64) {
      const bool on = j0 + lane < lb;
      const uint32_t w = on ? (uint32_t)col[sb + j0 + lane] : 0u;
      const bool take = on && pred(kb, w);
      const uint64_t bm = __ballot(take);
      if (take) emit(kb, bb, w, run + (uint32_t)__popcll(bm & below));
      run += (uint32_t)__popcll(bm);
    }
    if (lane == src) c = run;
  }
  __syncthreads();
  if (len > RCM_WAVE) s_long[__hip_atomic_fetch_add(&s_nlong, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = threadIdx.x;
  __syncthreads();
  const uint32_t nlong = s_nlong;
  for (uint32_t q = 0; q < nlong; q++) {   // (the same count in every thread; each turn ends on a barrier)
    const bool mine = s_long[q] == threadIdx.x;
    if (mine) { s_bring[0] = (uint32_t)s; s_bring[1] = (uint32_t)len; s_bring[2] = key; s_bring[3] = base; }
    __syncthreads();
    const int32_t sb = (int32_t)s_bring[0], lb = (int32_t)s_bring[1];
    const uint32_t kb = s_bring[2], bb = s_bring[3];
    uint32_t run = 0;
    for (int32_t j0 = 0; j0 < lb; j0 += WL_BS) {
      const bool on = j0 + (int32_t)threadIdx.x < lb;
      const uint32_t w = on ? (uint32_t)col[sb + j0 + (int32_t)threadIdx.x] : 0u;
      const bool take = on && pred(kb, w);
      const uint64_t bm = __ballot(take);
      if (lane == 0) s_wcnt[wv] = (uint32_t)__popcll(bm);
      __syncthreads();
      uint32_t before = 0, all = 0;
      for (int k = 0; k < WL_BS / 64; k++) { before += k < wv ? s_wcnt[k] : 0u; all += s_wcnt[k]; }
      if (take) emit(kb, bb, w, run + before + (uint32_t)__popcll(bm & below));
      run += all;
      __syncthreads();   // (s_wcnt and s_bring are read before the next turn writes them)
    }
    if (mine) c = run;
    __syncthreads();
  }
  return c;
}

// The exclusive prefix of c over the workgroup's threads, and the sum (convergent control flow only).
__device__ __forceinline__ uint32_t rcm_block_scan(uint32_t c, uint32_t *total) {
  __shared__ uint32_t s_w[WL_BS / 64];
  const int lane = wl_lane(), wv = (int)(threadIdx.x >> 6);
  uint32_t inc = c;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int k = 0; k < WL_BS / 64; k++) { before += k < wv ? s_w[k] : 0u; all += s_w[k]; }
  __syncthreads();
  *total = all;
  return before + inc - c;
}

// ---- thread 0 of the one workgroup that decides (rcm_begin, rcm_close) ----------------------------------------------------
// A sweep from src: a new generation, src alone in the level, the queue in the free part of order.
__device__ __forceinline__ void rcm_start_sweep(RcmCtl *ctl, const RcmState &St, uint32_t src) {
  const uint32_t gen = ctl->gen - 1u, d = ctl->done;
  ctl->gen = gen;
  St.stamp[src] = gen;
  St.order[d] = src;
  ctl->a = d; ctl->b = d + 1u; ctl->tail = d + 1u;
  ctl->xmin = RCM_NONE; ctl->xlast = src;
  ctl->lvl = 0; ctl->src = src; ctl->kind = 0;
}
// The numbering from r: r takes the next position.
__device__ __forceinline__ void rcm_start_numbering(RcmCtl *ctl, const RcmState &St, uint32_t r) {
  const uint32_t d = ctl->done;
  St.order[d] = r; St.posl[r] = (int32_t)d; St.levl[r] = 0;
  ctl->a = d; ctl->b = d + 1u; ctl->done = d + 1u;
  ctl->lvl = 0; ctl->kind = 1;
}
// The next component: the cursor advances to the next label without a position (the whole workgroup looks, 4 * WL_BS
// labels a turn), which becomes v; without sweeps the numbering starts from v, else the first sweep.  No label left:
// the run has finished.  (Convergent control flow only; posl is not written by this launch before the scan ends.)
__device__ __forceinline__ void rcm_next_component(RcmCtl *ctl, int32_t rows, const RcmState &St, int next_step) {
  __shared__ uint32_t s_cur, s_found;
  if (threadIdx.x == 0) { s_cur = ctl->done == (uint32_t)rows ? (uint32_t)rows : ctl->cursor; s_found = RCM_NONE; }
  __syncthreads();
  uint32_t found = RCM_NONE;
  for (int64_t cur = (int64_t)s_cur; cur < rows; cur += 4 * WL_BS) {
    uint32_t mine = RCM_NONE;
    for (int k = 0; k < 4; k++) {
      const int64_t l = cur + k * WL_BS + threadIdx.x;
      if (l < rows && St.posl[l] < 0) mine = min(mine, (uint32_t)l);
    }
    mine = wl_wave_min(mine);
    if (wl_lane() == 0 && mine != RCM_NONE) (void)__hip_atomic_fetch_min(&s_found, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    found = s_found;   // (written in this turn only when it was RCM_NONE before: nobody resets it)
    __syncthreads();
    if (found != RCM_NONE) break;
  }
  if (threadIdx.x != 0) return;
  if (found == RCM_NONE) { ctl->cursor = (uint32_t)rows; ctl->finished = 1; ctl->step = -1; return; }
  ctl->cursor = found;
  ctl->root = found; ctl->ecc = -1; ctl->left = ctl->sweeps;
  if (ctl->sweeps == 0) rcm_start_numbering(ctl, St, found);
  else rcm_start_sweep(ctl, St, found);
  ctl->step = next_step;
}

// ---- the launches of a call ---------------------------------------------------------------------------------------------
// Nothing numbered but the labels without an edge, which are their own components, first in the walk.
__global__ __launch_bounds__(WL_BS) void rcm_init(RcmGraph G, RcmState St, uint32_t zeros) {
  for (int64_t l = (int64_t)blockIdx.x * WL_BS + threadIdx.x; l < G.rows; l += (int64_t)gridDim.x * WL_BS) {
    St.stamp[l] = RCM_NONE; St.owner[l] = RCM_NONE;
    const bool lone = l < (int64_t)zeros;
    St.posl[l] = lone ? (int32_t)l : -1;
    St.levl[l] = lone ? 0 : -1;
    if (lone) St.order[l] = (uint32_t)l;
  }
}
// One workgroup, behind rcm_init's boundary (the host has zeroed the control block): the first component.
__global__ __launch_bounds__(WL_BS) void rcm_begin(RcmCtl *ctl, int32_t rows, RcmState St, uint32_t zeros, int32_t sweeps) {
  if (threadIdx.x == 0) {
    ctl->sweeps = sweeps; ctl->gen = RCM_NONE;
    ctl->done = zeros; ctl->cursor = zeros; ctl->components = (int32_t)zeros;
  }
  __syncthreads();
  rcm_next_component(ctl, rows, St, 0);
}

// Step s, kind 0: one level of a sweep.
__global__ __launch_bounds__(WL_BS) void rcm_sweep(RcmCtl *ctl, int s, RcmGraph G, RcmState St, WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->kind != 0) return;
  const int64_t a = (int64_t)ctl->a, b = (int64_t)ctl->b;
  const uint32_t gen = ctl->gen;
  uint32_t looked = 0, mn = RCM_NONE;
  for (int64_t t0 = a + (int64_t)blockIdx.x * WL_BS; t0 < b; t0 += (int64_t)gridDim.x * WL_BS) {
    const int64_t i = t0 + threadIdx.x;
    const bool valid = i < b;
    const int32_t v = valid ? (int32_t)St.order[i] : 0;
    const int32_t st = valid ? G.ptr[v] : 0;
    const int32_t len = valid ? G.ptr[v + 1] - st : 0;
    looked += (uint32_t)len;
    (void)rcm_tile(G.col, valid, 0u, 0u, st, len,
        [&](uint32_t, uint32_t w) {   // (an older generation is a larger word; the one lane that reads it owns w)
          return wl_load(&St.stamp[w]) != gen && __hip_atomic_fetch_min(&St.stamp[w], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen;
        },
        [&](uint32_t, uint32_t, uint32_t w, uint32_t) {
          St.order[wl_append_here(&ctl->tail)] = w;
          mn = min(mn, w);
        });
  }
  mn = wl_wave_min(mn);
  if (wl_lane() == 0 && mn != RCM_NONE) (void)__hip_atomic_fetch_min(&ctl->xmin, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  wl_block_part(part, 0u, looked);
}

// Step s, kind 1: every unnumbered entry of the level's lists goes to the smallest position that has it.
__global__ __launch_bounds__(WL_BS) void rcm_claim(const RcmCtl *ctl, int s, RcmGraph G, RcmState St) {
  if (ctl->step != s || ctl->kind != 1) return;
  const int64_t a = (int64_t)ctl->a, b = (int64_t)ctl->b;
  for (int64_t t0 = a + (int64_t)blockIdx.x * WL_BS; t0 < b; t0 += (int64_t)gridDim.x * WL_BS) {
    const int64_t i = t0 + threadIdx.x;
    const bool valid = i < b;
    const int32_t v = valid ? (int32_t)St.order[i] : 0;
    const int32_t st = valid ? G.ptr[v] : 0;
    const int32_t len = valid ? G.ptr[v + 1] - st : 0;
    (void)rcm_tile(G.col, valid, (uint32_t)i, 0u, st, len,
        [&](uint32_t, uint32_t w) { return St.posl[w] < 0; },   // (posl is not written in this launch)
        [&](uint32_t key, uint32_t, uint32_t w, uint32_t) {
          if (wl_load(&St.owner[w]) > key) (void)__hip_atomic_fetch_min(&St.owner[w], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
  }
}

// The positions of workgroup k of a numbering level: a contiguous chunk of [a, b).
__device__ __forceinline__ void rcm_chunk(int64_t a, int64_t b, int64_t *lo, int64_t *hi) {
  const int64_t chunk = (b - a + gridDim.x - 1) / gridDim.x;
  *lo = min(b, a + (int64_t)blockIdx.x * chunk);
  *hi = min(b, *lo + chunk);
}

// Step s, kind 1: cnt[i] = the children of position i; the workgroup's total and its list entries -> its WlPart.
__global__ __launch_bounds__(WL_BS) void rcm_count(const RcmCtl *ctl, int s, RcmGraph G, RcmState St, WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->kind != 1) return;
  int64_t lo, hi;
  rcm_chunk((int64_t)ctl->a, (int64_t)ctl->b, &lo, &hi);
  uint32_t total = 0, looked = 0;
  for (int64_t t0 = lo; t0 < hi; t0 += WL_BS) {
    const int64_t i = t0 + threadIdx.x;
    const bool valid = i < hi;
    const int32_t v = valid ? (int32_t)St.order[i] : 0;
    const int32_t st = valid ? G.ptr[v] : 0;
    const int32_t len = valid ? G.ptr[v + 1] - st : 0;
    looked += (uint32_t)len;
    const uint32_t c = rcm_tile(G.col, valid, (uint32_t)i, 0u, st, len,
        [&](uint32_t key, uint32_t w) { return St.owner[w] == key; },   // (owner is not written in this launch)
        [&](uint32_t, uint32_t, uint32_t, uint32_t) {});
    if (valid) St.cnt[i] = c;
    total += c;
  }
  wl_block_part(part, total, looked);
}

// Step s, kind 1: the children of position i stand at b + (the children of the positions before i) + their rank.
__global__ __launch_bounds__(WL_BS) void rcm_place(const RcmCtl *ctl, int s, RcmGraph G, RcmState St, const WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->kind != 1) return;
  int64_t lo, hi;
  rcm_chunk((int64_t)ctl->a, (int64_t)ctl->b, &lo, &hi);
  if (lo >= hi) return;   // (the same in every thread)
  const int32_t next_level = ctl->lvl + 1;
  uint32_t before = 0, all;
  for (int k = (int)threadIdx.x; k < (int)blockIdx.x; k += WL_BS) before += part[k].a;
  (void)rcm_block_scan(before, &all);   // the children of the workgroups before this one
  uint32_t at = ctl->b + all;
  for (int64_t t0 = lo; t0 < hi; t0 += WL_BS) {
    const int64_t i = t0 + threadIdx.x;
    const bool valid = i < hi;
    const int32_t v = valid ? (int32_t)St.order[i] : 0;   // (order[a, b) is not written in this launch: the children go behind b)
    const int32_t st = valid ? G.ptr[v] : 0;
    const int32_t len = valid ? G.ptr[v + 1] - st : 0;
    uint32_t tile_total;
    const uint32_t mine = rcm_block_scan(valid ? St.cnt[i] : 0u, &tile_total);
    (void)rcm_tile(G.col, valid, (uint32_t)i, at + mine, st, len,
        [&](uint32_t key, uint32_t w) { return St.owner[w] == key; },
        [&](uint32_t, uint32_t base, uint32_t w, uint32_t rank) {
          const uint32_t p = base + rank;
          St.order[p] = w; St.posl[w] = (int32_t)p; St.levl[w] = next_level;
        });
    at += tile_total;
  }
}

// Closes step s (slot r of the batch).  One workgroup folds the WlParts and its first thread records the step and decides.
__global__ __launch_bounds__(WL_BS) void rcm_close(RcmCtl *ctl, int r, int s, int32_t rows, int nparts, const WlPart *__restrict__ part, RcmState St) {
  __shared__ int32_t s_next;   // thread 0's verdict, across the barrier below: the component is numbered, look for the next
  if (!wl_from_thread0(ctl->step == s)) return;
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x == 0) {
    const uint32_t children = sums.a, looked = sums.b;
    s_next = 0;
    const int kind = ctl->kind;
    const uint32_t b = ctl->b;
    ctl->rec[r] = RcmRec{1, kind, b - ctl->a, looked};
    if (kind == 0) {
      const uint32_t tail = ctl->tail;
      if (tail > b) {   // the next level of the sweep
        ctl->a = b; ctl->b = tail;
        ctl->xlast = ctl->xmin; ctl->xmin = RCM_NONE;
        ctl->lvl += 1;
      } else {          // the sweep from src has ended: its eccentricity is lvl, x the smallest label of its last level
        ctl->sweeps_run += 1;
        bool go_on = true;
        if (ctl->ecc < 0) ctl->ecc = ctl->lvl;                                         // (the sweep from v: r = v)
        else if (ctl->lvl > ctl->ecc) { ctl->root = ctl->src; ctl->ecc = ctl->lvl; }   // x is the better root
        else go_on = false;
        const uint32_t x = ctl->xlast;
        if (go_on && x != ctl->root && ctl->left > 0) { ctl->left -= 1; rcm_start_sweep(ctl, St, x); }
        else rcm_start_numbering(ctl, St, ctl->root);
      }
      ctl->step = s + 1;
    } else if (children > 0) {   // the next level of the numbering
      ctl->a = b; ctl->b = b + children; ctl->done = b + children;
      ctl->lvl += 1;
      ctl->step = s + 1;
    } else {                     // the component is numbered
      ctl->components += 1;
      s_next = 1;
    }
  }
  __syncthreads();
  if (s_next) rcm_next_component(ctl, rows, St, s + 1);
}

// The closing launch: perm, pos and level through S, and the workgroup's share of bandwidth and profile under the identity
// and under the new order.  Position k becomes rows - 1 - k when `reverse`.  The places of perm beyond `done` get -1, and
// so do pos and level of the vertices without a position (a run cut short).
__global__ __launch_bounds__(WL_BS) void rcm_finish(const RcmCtl *ctl, RcmGraph G, RcmState St, const int32_t *__restrict__ S, int32_t reverse,
                                                     int32_t *__restrict__ perm, int32_t *__restrict__ pos, int32_t *__restrict__ level,
                                                     RcmFin *__restrict__ fin) {
  const int lane = wl_lane();
  const int64_t rows = G.rows, done = (int64_t)ctl->done;
  const auto placed = [&](int32_t p) { return p < 0 ? -1 : reverse ? (int32_t)(rows - 1 - p) : p; };
  uint32_t bw0 = 0, bw1 = 0;
  uint64_t prof0 = 0, prof1 = 0;
#pragma unroll 1
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const int64_t l = base + lane;
    const bool on = l < rows;
    if (on) {   // as a position, and as a label
      perm[placed((int32_t)l)] = l < done ? S[St.order[l]] : -1;
      if (pos) pos[S[l]] = placed(St.posl[l]);
      if (level) level[S[l]] = St.levl[l];
    }
    const int32_t st = on ? G.ptr[l] : 0;
    const int32_t len = on ? G.ptr[l + 1] - st : 0;
    const int32_t v = on ? S[l] : 0, p = on ? placed(St.posl[l]) : 0;
    int32_t vmin = v, pmin = p;
    if (len <= RCM_LANE)
#pragma unroll 1
      for (int32_t j = 0; j < len; j++) {   // (unrolled further, the loads of S and posl in flight take more than 128 VGPRs)
        const int32_t lw = G.col[st + j];
        const int32_t u = S[lw], q = placed(St.posl[lw]);
        vmin = min(vmin, u); pmin = min(pmin, q);
        bw0 = max(bw0, (uint32_t)abs(v - u)); bw1 = max(bw1, (uint32_t)abs(p - q));
      }
    uint64_t m = __ballot(len > RCM_LANE);
#pragma unroll 1
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(st, src), lb = __shfl(len, src), vb = __shfl(v, src), pb = __shfl(p, src);
      int32_t um = vb, qm = pb;
#pragma unroll 1
      for (int32_t j = lane; j < lb; j += 64) {
        const int32_t lw = G.col[sb + j];
        const int32_t u = S[lw], q = placed(St.posl[lw]);
        um = min(um, u); qm = min(qm, q);
        bw0 = max(bw0, (uint32_t)abs(vb - u)); bw1 = max(bw1, (uint32_t)abs(pb - q));
      }
      um = wl_wave_fold<WlMin>(um); qm = wl_wave_fold<WlMin>(qm);
      if (lane == src) { vmin = um; pmin = qm; }
    }
    if (on) { prof0 += (uint64_t)(v - vmin); prof1 += (uint64_t)(p - pmin); }
  }
  // (four folds one after the other, left to right, each with its pair of barriers: once per call, so it does not matter)
  const RcmFin f{{wl_block_fold<WlMax>(bw0), wl_block_fold<WlMax>(bw1)}, {wl_block_fold<WlSum>(prof0), wl_block_fold<WlSum>(prof1)}, 0ull};
  if (threadIdx.x == 0) fin[blockIdx.x] = f;
}
// One workgroup folds the RcmFins into the control block.
__global__ __launch_bounds__(WL_BS) void rcm_total(RcmCtl *ctl, int nparts, const RcmFin *__restrict__ fin) {
  RcmFin f = {};
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS)
    for (int k = 0; k < 2; k++) { f.bw[k] = max(f.bw[k], fin[i].bw[k]); f.prof[k] += fin[i].prof[k]; }
  for (int k = 0; k < 2; k++) {   // (four folds one after the other, as in rcm_finish)
    const uint32_t bw = wl_block_fold<WlMax>(f.bw[k]);
    const uint64_t prof = wl_block_fold<WlSum>(f.prof[k]);
    if (threadIdx.x == 0) { ctl->bw[k] = (int64_t)bw; ctl->prof[k] = (int64_t)prof; }
  }
}

} // namespace sh
