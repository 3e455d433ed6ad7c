// msf.hip.h -- kernels of sh_msf: the minimum spanning forest of the simple undirected graph under a square matrix, the
// values as weights, by Boruvka rounds on a parent forest over a flat list of edges (Boruvka, "O jistem problemu
// minimalnim", 1926; on a GPU: Vineet, Harish, Patidar, Narayanan, "Fast minimum spanning tree for large graphs on the
// GPU", HPG 2009).  in_msf[e] becomes 1 for the edges of the forest, comp[v] the largest vertex index of v's component
// (DESIGN.md "6m Minimum spanning forest").
//
// Weights are float32 compared by the total order of their bit patterns: with b the bits, k(b) = b ^ 0xFFFFFFFF if the
// sign bit is set, else b ^ 0x80000000 (-NaN < -inf < ... < -0.0 < denormals < ... < +inf < +NaN).  The weight of edge
// {u, v} is the smallest, by k, over all counting entries (u, v) and (v, u).  KEY(e) = k(weight[e]) << 32 | e: NO TWO
// KEYS ARE EQUAL, so the forest is unique -- it is what Kruskal's algorithm returns when it takes the edges in ascending
// KEY -- and every result is compared with ==.  No key is MSF_MAX (e < 2^31).
//
// State: p[v] the parent word, best[v] one 64-bit word per vertex, to[v] the root that a root will hook to, eu[M] / ev[M]
// / wk[M] the ends (eu < ev) and k(weight) of every edge, two work lists of M edge ids.  AT THE START OF EVERY ROUND EVERY
// TREE IS A STAR: p[v] is a root for all v.  Round 1 has p[v] = v and the list holds all M edges.  The work item is an
// edge of a flat list: there are no long rows and no pieces, every lane gets one edge.  A ROUND is one step of the control
// block, a fixed set of launches, each of which returns at once unless the control block gives it work:
//   msf_find   best[.] = MSF_MAX was written by a launch that ended before this one.  For every edge e of the list,
//              a = p[eu[e]] and b = p[ev[e]].  a == b: the edge is inside a tree for good and is dropped.  Otherwise it is
//              appended to the next list with a wave-aggregated push, and KEY(e) goes into best[a] and best[b] with one
//              64-bit atomic minimum each (one global_atomic_umin_x2: no compare-and-swap loop).  The atomic is issued
//              only if KEY(e) is below a load of the word: the word only falls, so a stale read can only let a needless
//              atomic through and never suppresses a needed one.
//   msf_pick   every root r with best[r] != MSF_MAX takes e = the low 32 bits, stores in_msf[e] = 1 (two roots that chose
//              the same edge store the same value), finds the other root o among p[eu[e]] and p[ev[e]] and writes
//              to[r] = o -- except in a mutual pair with r > o: when best[o] == best[r] the smaller index hooks and the
//              larger stays a root (to[r] = r).  PICK READS p AND WRITES ONLY to AND in_msf: the launch that decides the
//              hooks must not read a word that the same launch writes (a root reading p[u] while u's own lane stores p[u]
//              would take the wrong other root).
//   msf_link   p[r] = to[r] for every root that picked; the same lane puts best[r] back to MSF_MAX (it is the only one
//              that looks at the word in this launch), so the next round's find meets MSF_MAX everywhere.
//   msf_jump   MSF_SWEEPS launches over all vertices, at most MSF_JUMPS stores of p[v] = p[p[v]] per vertex each; sweep
//              i > 0 returns at once unless sweep i - 1 moved a pointer.  The bound holds for ANY ORDER OF THE LANES: a lane
//              that runs before the vertices above it sees old pointers and gains only one hop per jump, so a launch
//              shortens a depth d to at most ceil(d / (MSF_JUMPS + 1)), not to d / 2^MSF_JUMPS.  (MSF_JUMPS + 1)^MSF_SWEEPS
//              >= 2^31 > rows (the static_assert below): every tree is a star again when the round ends, on any input and
//              any schedule.
//   msf_close  sums the workgroups' counts, records the round, swaps the lists.  The run finishes when FIND KEPT NO
//              EDGE.  (pick, link and the jumps return at once in that round: nothing was put into best.)
// After the last round msf_top takes top[root] = max v by an atomic maximum (top lives in best's memory, which holds
// nothing then), and msf_label writes comp[v] = top[p[v]] and counts the roots.
//
// Why that is right.  All keys differ, so the lightest edge leaving a tree is in the one minimum spanning forest (the cut
// property), whatever the other trees do in that round.  In the graph "root -> chosen other root" every cycle has length
// 2: along a cycle the chosen keys would have to fall strictly unless both ends chose one edge; the mutual rule breaks
// exactly those cycles, so link builds a forest.  Pointers never leave a component.  A run ends when no listed edge joins
// two trees; dropped edges were inside a tree and trees only merge, so every component is one star.
//
// find sees one state, so the set of kept edges, best, the hooks, the rounds, walked (the list length at the start), kept
// and hooks (to pointers applied) of every round are functions of the input alone; only the order inside a list, the
// jumps and the times may differ from run to run.  Every tree with a leaving edge merges: a run has at most
// floor(log2(rows)) + 1 rounds, the empty last one included.
//
// Invariant 1: NO LIST CAN OVERFLOW ON ANY INPUT.  An edge enters a list once per round, by the one lane that holds it:
// M places suffice.
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE, and no lane for another lane's.  There is no
// compare-and-swap, no retry and no spin loop: a jump loop ends after MSF_JUMPS stores, the gate words a launch reads
// were written by a launch that ended before it.  Values are written with vector stores or plain C++ only.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int MSF_BATCH = 32;            // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int MSF_MAX_BLOCKS = 1024;     // workgroups of a launch at most: two WlParts each
constexpr int MSF_CTL_BYTES = 1024;      // device bytes set aside for MsfCtl
constexpr int MSF_PART_BYTES = 16 * MSF_MAX_BLOCKS;
constexpr int MSF_JUMPS = 16;            // a jumping launch: jumps per vertex at most
constexpr int MSF_SWEEPS = 8;            // jumping launches of a round
constexpr uint64_t MSF_MAX = 0xFFFFFFFFFFFFFFFFull;   // no key

constexpr uint64_t msf_pow(uint64_t b, int n) { return n == 0 ? 1ull : b * msf_pow(b, n - 1); }
static_assert(msf_pow(MSF_JUMPS + 1, MSF_SWEEPS) >= (1ull << 31),
              "(MSF_JUMPS + 1)^MSF_SWEEPS >= 2^31: the sweeps of a round make a star of a chain of any depth below 2^31");

struct MsfRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran;
  uint32_t walked, kept, hooks, jumps, pad;
};
// Control block in device memory.
struct MsfCtl {
  uint32_t n[2];                 // the lengths of work list 0 / 1
  int32_t p;                     // the list the next round walks (the other one is filled meanwhile)
  int32_t step;                  // the round that runs next (-1 once the run has finished)
  int32_t finished;
  uint32_t rows, components, pad;
  uint32_t moved[MSF_SWEEPS];    // jumping launch i of the open round changed a pointer
  MsfRec rec[MSF_BATCH];
};
// The WlParts of a workgroup.  msf_link: a = hooks.  Jumping launches (an array of their own): a = pointers changed,
// added up over the round's launches.

struct MsfEdges {   // the handle's edge arrays, as a kernel argument
  int32_t M;
  const int32_t *eu, *ev;
  const uint32_t *wk;
};
struct MsfLists { uint32_t *list[2]; };

// k(b) and its inverse
__device__ __forceinline__ uint32_t msf_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u); }
__device__ __forceinline__ uint32_t msf_unkey(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// (a load that goes to the L2, where the atomics meet: a line of this CU's cache may be older, which is allowed but
// would let more needless atomics through)
__device__ __forceinline__ uint64_t msf_load(const uint64_t *w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void msf_lower(uint64_t *w, uint64_t key) {
  if (key < msf_load(w)) (void)__hip_atomic_fetch_min(w, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Building the handle (once): entry j of the arrays as given takes the atomic minimum of k(val[j]) into wk[e], e the
// edge it stands for -- the edge rule applied again (wl_und_flag's), the row by bisection of row_ptr (wl_row_of), the pair
// (min, max) by bisection of the M edges eu / ev, which hold it.  wk was filled with 0xFFFFFFFF by the host.
__global__ __launch_bounds__(WL_BS) void msf_weights(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                     const uint32_t *__restrict__ val, int64_t nnz, int32_t rows,
                                                     const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, int64_t m,
                                                     uint32_t *__restrict__ wk) {
  const int64_t j = (int64_t)blockIdx.x * WL_BS + threadIdx.x;
  if (j >= nnz) return;
  const int32_t c = col_idx[j];
  const uint32_t bits = val[j];
  if (bits == 0u || (uint32_t)c >= (uint32_t)rows) return;
  const int32_t r = wl_row_of(row_ptr, rows, j);
  if (c == r) return;
  const int32_t a = min(r, c), b = max(r, c);
  int64_t lo = 0, hi = m;   // the first edge that is not below (a, b)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (eu[mid] < a || (eu[mid] == a && ev[mid] < b)) lo = mid + 1; else hi = mid;
  }
  (void)__hip_atomic_fetch_min(&wk[min(lo, m - 1)], msf_key(bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Every vertex a tree of its own, no key anywhere, list 0 = all edges, no edge chosen; weight[e] (if wanted) = the bits
// of the entry that gave wk[e].  (The host has zeroed the control block: step = 0, p = 0.)
__global__ __launch_bounds__(WL_BS) void msf_init(MsfCtl *ctl, int32_t rows, MsfEdges E, uint32_t *__restrict__ p,
                                                  uint64_t *__restrict__ best, uint32_t *__restrict__ list0,
                                                  int32_t *__restrict__ in_msf, uint32_t *__restrict__ weight) {
  const int64_t n = max(rows, E.M);
  for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WL_BS) {
    if (i < rows) { p[i] = (uint32_t)i; best[i] = MSF_MAX; }
    if (i < E.M) {
      list0[i] = (uint32_t)i;
      in_msf[i] = 0;
      if (weight) weight[i] = msf_unkey(E.wk[i]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->rows = (uint32_t)rows; ctl->n[0] = (uint32_t)E.M; }
}

// Round s: the edges of the list that still join two trees go on to the next list and bid for both trees.
__global__ __launch_bounds__(WL_BS) void msf_find(MsfCtl *ctl, int s, MsfEdges E, const uint32_t *__restrict__ p, uint64_t *best,
                                                  MsfLists L) {
  if (ctl->step != s) return;
  const int pl = ctl->p, q = pl ^ 1;
  const int64_t n = ctl->n[pl];
  const uint32_t *__restrict__ list = L.list[pl];
  uint32_t *__restrict__ next = L.list[q];
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const uint32_t e = valid ? list[base + lane] : 0u;
    const uint32_t a = valid ? p[E.eu[e]] : 0u, b = valid ? p[E.ev[e]] : 0u;
    const bool keep = valid && a != b;
    const uint32_t at = wl_wave_append(&ctl->n[q], keep, lane);
    if (keep) {   // (only this lane holds e in this round: invariant 1)
      next[at] = e;
      const uint64_t key = ((uint64_t)E.wk[e] << 32) | (uint64_t)e;
      msf_lower(&best[a], key);
      msf_lower(&best[b], key);
    }
  }
}

// Round s: every root with a key chooses its edge and the root it will hook to.  Reads p and best, writes to and in_msf.
__global__ __launch_bounds__(WL_BS) void msf_pick(const MsfCtl *ctl, int s, int32_t rows, MsfEdges E, const uint32_t *__restrict__ p,
                                                  const uint64_t *__restrict__ best, uint32_t *__restrict__ to,
                                                  int32_t *__restrict__ in_msf) {
  if (ctl->step != s || ctl->n[ctl->p ^ 1] == 0u) return;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    const uint64_t k = best[v];
    if (k == MSF_MAX) continue;   // (find bids for roots only: v is a root)
    const uint32_t e = (uint32_t)k;
    in_msf[e] = 1;
    const uint32_t a = p[E.eu[e]], b = p[E.ev[e]];
    const uint32_t o = a == (uint32_t)v ? b : a;
    to[v] = (best[o] == k && (uint32_t)v > o) ? (uint32_t)v : o;
  }
}

// Round s: the hooks.  A lane reads and writes the words of its own vertex only.
__global__ __launch_bounds__(WL_BS) void msf_link(const MsfCtl *ctl, int s, int32_t rows, uint32_t *__restrict__ p,
                                                  uint64_t *__restrict__ best, const uint32_t *__restrict__ to,
                                                  WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->n[ctl->p ^ 1] == 0u) return;
  uint32_t hooks = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    if (best[v] == MSF_MAX) continue;
    best[v] = MSF_MAX;
    const uint32_t t = to[v];
    if (t != (uint32_t)v) { p[v] = t; hooks++; }
  }
  wl_block_part(part, hooks, 0u);
}

// Jumping launch i of round s, over all vertices: wl_jump, MSF_JUMPS jumps per vertex at most.  Every jump gains at
// least one hop of the forest the launch started from.
__global__ __launch_bounds__(WL_BS) void msf_jump(MsfCtl *ctl, int s, int i, int32_t rows, uint32_t *p, WlPart *__restrict__ jpart) {
  if (ctl->step != s || ctl->n[ctl->p ^ 1] == 0u || (i > 0 && !ctl->moved[i - 1])) return;
  wl_jump(i, MSF_JUMPS, rows, p, jpart, ctl->moved);
}

// Closes round s (slot k of the batch).  One workgroup sums the WlParts (no atomics on one word) and its first lane
// records the round, swaps the lists and decides.
__global__ __launch_bounds__(WL_BS) void msf_close(MsfCtl *ctl, int k, int s, int nparts, const WlPart *__restrict__ part,
                                                   const WlPart *__restrict__ jpart) {
  if (!wl_from_thread0(ctl->step == s)) return;
  const int pl = ctl->p, q = pl ^ 1;
  const uint32_t kept = ctl->n[q];
  uint32_t hooks = 0, jumps = 0;   // hooks, pointers changed (the parts are this round's only if its launches ran)
  if (kept)
    for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) { hooks += part[i].a; jumps += jpart[i].a; }
  hooks = wl_block_fold<WlSum>(hooks);
  jumps = wl_block_fold<WlSum>(jumps);
  if (threadIdx.x != 0) return;
  ctl->rec[k] = MsfRec{1, ctl->n[pl], kept, hooks, jumps, 0u};
  ctl->n[pl] = 0u;
  ctl->p = q;
  for (int i = 0; i < MSF_SWEEPS; i++) ctl->moved[i] = 0u;
  if (kept == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = s + 1;
}

// After a complete run (every tree a star): top[root] = the largest index of the tree (top zeroed by the host).  The
// vertices are taken from the largest down, so that all but the first lanes to arrive find the word at or above their
// index and issue nothing; a wave whose lanes share one root sends its largest index alone.
__global__ __launch_bounds__(WL_BS) void msf_top(int32_t rows, const uint32_t *__restrict__ p, uint32_t *top) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < rows; base += wl_waves() * 64) {
    const bool valid = base + lane < rows;
    const uint32_t v = (uint32_t)(rows - 1 - (base + lane));   // (lane 0 is valid and holds the wave's largest index)
    const uint32_t r = valid ? p[v] : 0u;
    const uint32_t r0 = (uint32_t)__shfl((int)r, 0);
    const bool same = __ballot(valid && r != r0) == 0ull;
    if (valid && (!same || lane == 0) && __hip_atomic_load(&top[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
      (void)__hip_atomic_fetch_max(&top[r], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Closes the call: comp[v] (if wanted) = top[p[v]], or -1 everywhere after a run cut short (a half-built forest is no
// partition), and the number of roots: the components, or after a run cut short the trees so far.
__global__ __launch_bounds__(WL_BS) void msf_label(MsfCtl *ctl, int32_t rows, int complete, const uint32_t *__restrict__ p,
                                                   const uint32_t *__restrict__ top, int32_t *__restrict__ comp) {
  uint32_t roots = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    const uint32_t up = p[v];
    if (comp) comp[v] = complete ? (int32_t)top[up] : -1;
    roots += up == (uint32_t)v ? 1u : 0u;
  }
  roots = wl_block_fold<WlSum>(roots);
  if (threadIdx.x == 0 && roots) wl_add(&ctl->components, roots);   // (one add per workgroup)
}

} // namespace sh
