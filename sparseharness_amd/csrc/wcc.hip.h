// wcc.hip.h -- kernels of sh_wcc: weakly connected components by hooking roots and pointer jumping, with a sampled skip
// of the largest tree (hooking and jumping: Shiloach, Vishkin, "An O(log n) parallel connectivity algorithm", J.
// Algorithms 1982; neighbour sampling and the skip: Sutton, Ben-Nun, Barak, "Optimizing parallel graph connectivity
// computation via subgraph sampling", IPDPS 2018).  comp[v] becomes the largest vertex index of v's weak component
// (DESIGN.md "6h Weakly connected components").
//
// The graph lives in the layout of sh_bfs_graph (in_ptr / in_col: the edges c -> r by row r; out_ptr / out_row: by source
// vertex c); the direction of an edge is ignored.  The state is one parent word p[v] per vertex with p[v] >= v ALWAYS:
// pointers only go to larger indices, so there are no cycles, and a root (p[r] == r) is the largest index of its tree.
// A HOOK is a compare-and-swap on a ROOT: p[lo] goes from lo to hi, lo < hi, lo a root and hi a vertex of another tree
// (hi > lo, and lo is the largest index of its own).  A JUMP is p[v] = p[p[v]].  Neither moves a vertex out of its tree:
// TREES ONLY EVER MERGE, NEVER SPLIT.  (An atomic max on the pointer of a non-root could tear a tree apart; it is not
// used.)  A ROUND is one step of the control block, a fixed set of launches:
//   wcc_sample   round j < sample: every vertex hooks along the j-th stored entry of its row, if it has one.
//   wcc_compact  round `sample`, before its walk: L = the most frequent parent among 1024 evenly spaced vertices (ties
//                to the larger index); S = { v : p[v] == L } is fixed here, once; every vertex outside S joins the work
//                list and the pieces of its long in- and out-list join the two piece lists.  sample == 0: S is empty.
//   wcc_full     rounds >= sample: wl_expand over the work list's in-lists and over its out-lists hooks the two ends of
//                every entry.  (An edge with one end in S is stored in the row of either end, and only the other end
//                walks: hence both lists.  Edges inside S are never looked at: their ends are in one tree for good.)
//   wcc_jump     WCC_SWEEPS launches over ALL rows, members of S included; sweep i > 0 returns at once unless sweep i - 1
//                changed a pointer.  At most WCC_JUMPS jumps per vertex per launch.
//   wcc_decide   sums the WlParts, records the round and finishes when a full round found every walked entry with both
//                ends under one parent, hooked nothing and jumped nothing.
// wcc_label closes the call: comp[v] = p[v] (or -1 everywhere after an incomplete run) and the roots are counted.
//
// Why that is right: pointers never leave a component (a hook follows an edge, a jump stays in the tree).  In the last
// round nothing was written, so what its launches saw is one state: every tree a star (no jump was possible) and every
// walked entry with both ends under one root.  S sits in one tree.  Every edge is walked or lies inside S, so a
// component is one star, and its root is its largest index.
//
// Invariant 1: NO LIST CAN OVERFLOW ON ANY INPUT.  A vertex enters the work list at most once per call, in wcc_compact,
// by the one lane that looks at it: `rows` places suffice, and each piece list is bounded by edges / (WCC_PIECE / 2) + 1
// (wl_push_pieces).
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE, and no lane for another lane's.  There is no spin loop:
// a hook climbs and retries at most WCC_HOPS times and then leaves the entry to the next round (it is counted as
// unsettled, so the run cannot finish over it); a failed compare-and-swap continues from the word it returned; a jump
// loop ends after WCC_JUMPS stores; the gate words a launch reads were written by a launch that ended before it.
// Values are written with vector stores or plain C++ only.  Lanes of one launch race on p in one direction only
// (pointers grow along their tree's path to the root): a stale word is an older ancestor and costs a later round,
// never a wrong answer.  max_rounds bounds the call.
//
// Work distribution as worklist.hip.h describes it.  The handle is built by its kernels (wl_edge_flag<BfsKeep>, ...).
#pragma once
#include "bfs.hip.h"
#include "worklist.hip.h"

namespace sh {

constexpr int WCC_SHORT = 8;             // lists up to this many edges: one lane each
constexpr int WCC_PIECE = 2048;          // lists above this are walked in pieces of this many edges
constexpr int WCC_ROW_PIECE = 4096;      // the shared builder's static row pieces (the search does not use them)
constexpr int WCC_BATCH = 32;            // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int WCC_MAX_BLOCKS = 1024;     // workgroups of a launch at most: two WlParts each
constexpr int WCC_CTL_BYTES = 2048;      // device bytes set aside for WccCtl
constexpr int WCC_PART_BYTES = 16 * WCC_MAX_BLOCKS;
constexpr int WCC_HOPS = 8;              // a hook: climbs and retries per entry at most
constexpr int WCC_JUMPS = 8;             // a jumping launch: jumps per vertex at most
constexpr int WCC_SWEEPS = 6;            // jumping launches of a round
constexpr int WCC_PICKS = 1024;          // vertices the pick looks at
constexpr uint32_t WCC_NONE = 0xFFFFFFFFu;   // no vertex (rows < 2^31)

enum : int32_t { WCC_KIND_SAMPLE = 0, WCC_KIND_FULL = 1 };   // kind_per_round

struct WccRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran, kind;
  uint32_t hooks, jumps, edges;
};
// Control block in device memory.
struct WccCtl {
  uint32_t n, nip, nop;          // length of the work list, of its in-list pieces, of its out-list pieces
  int32_t step;                  // the round that runs next (-1 once the run has finished)
  int32_t finished;
  int32_t sample;                // the caller's setting
  uint32_t rows, skipped, components;
  uint32_t moved[WCC_SWEEPS];    // jumping launch i of the open round changed a pointer
  WccRec rec[WCC_BATCH];
};
// The WlParts of a workgroup.  Hooking launch: a = entries looked at, b = hooks, c = entries left unsettled.  Jumping
// launches (an array of their own): a = pointers changed, added up over the round's launches.

struct WccGraph {   // the handle's edge lists, as a kernel argument
  int32_t rows;
  const int32_t *in_ptr, *in_col, *out_ptr, *out_row;
};

// The two ends u, w of an entry: are they under one parent; if not, hook.  -> 0 settled (one tree), 1 hooked, 2 left to
// the next round.  `a` and `b` are ancestors (or selves) of u and w throughout; only the smaller is ever climbed or
// hooked, and it is hooked only while it is a root.
__device__ __forceinline__ int wcc_hook(uint32_t *p, uint32_t u, uint32_t w) {
  uint32_t a = p[u], b = p[w];
  uint32_t seen = WCC_NONE;   // p[lo] as a failed compare-and-swap returned it (L2's word, not a stale line of this CU)
  for (int h = 0; h < WCC_HOPS; h++) {
    if (a == b) return 0;
    const uint32_t lo = min(a, b), hi = max(a, b);
    const uint32_t up = seen != WCC_NONE ? seen : p[lo];
    seen = WCC_NONE;
    if (up != lo) {   // lo is no root: climb
      if (a == lo) a = up; else b = up;
      continue;
    }
    uint32_t expect = lo;
    if (__hip_atomic_compare_exchange_strong(&p[lo], &expect, hi, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return 1;
    seen = expect;   // (somebody else hooked lo: expect > lo now)
  }
  return a == b ? 0 : 2;
}

// p[v] = v for every row; the caller's setting into the control block (which the host has zeroed: step = 0)
__global__ __launch_bounds__(WL_BS) void wcc_init(WccCtl *ctl, int32_t rows, int32_t sample, uint32_t *__restrict__ p) {
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) p[v] = (uint32_t)v;
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->rows = (uint32_t)rows; ctl->sample = sample; }
}

// Sampling round s: every vertex hooks along entry s of its row.
__global__ __launch_bounds__(WL_BS) void wcc_sample(const WccCtl *ctl, int s, WccGraph G, uint32_t *p, WlPart *__restrict__ part) {
  if (ctl->step != s || s >= ctl->sample) return;
  uint32_t looked = 0, hooks = 0, open = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < G.rows; v += (int64_t)gridDim.x * WL_BS) {
    const int32_t b = G.in_ptr[v];
    if (G.in_ptr[v + 1] - b <= s) continue;
    const int r = wcc_hook(p, (uint32_t)G.in_col[b + s], (uint32_t)v);
    looked++; hooks += r == 1; open += r != 0;
  }
  wl_block_part<WlSum, WlSum>(part, looked, hooks, open);
}

// L = the most frequent parent among the WCC_PICKS vertices i * rows / WCC_PICKS, ties to the larger index -> every
// thread (convergent control flow only).  Counted exactly in a table of twice as many slots in LDS (open addressing; a
// probe sequence is bounded by the table, which can never fill), so L depends on the forest alone.
__device__ __forceinline__ uint32_t wcc_pick(const uint32_t *__restrict__ p, int32_t rows) {
  constexpr int SLOTS = 2 * WCC_PICKS;
  __shared__ uint32_t s_key[SLOTS], s_cnt[SLOTS];
  for (int i = (int)threadIdx.x; i < SLOTS; i += WL_BS) { s_key[i] = WCC_NONE; s_cnt[i] = 0u; }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < WCC_PICKS; i += WL_BS) {
    const uint32_t r = p[(int64_t)i * rows / WCC_PICKS];
    uint32_t h = (r * 2654435761u) >> 21;   // 11 bits
    for (int probe = 0; probe < SLOTS; probe++) {
      const uint32_t old = atomicCAS(&s_key[h], WCC_NONE, r);
      if (old == WCC_NONE || old == r) { atomicAdd(&s_cnt[h], 1u); break; }
      h = (h + 1u) & (uint32_t)(SLOTS - 1);
    }
  }
  __syncthreads();
  uint64_t best = 0;   // count << 32 | vertex: the larger count, ties to the larger vertex, is the larger word
  for (int i = (int)threadIdx.x; i < SLOTS; i += WL_BS)
    if (s_key[i] != WCC_NONE) best = max(best, ((uint64_t)s_cnt[i] << 32) | (uint64_t)s_key[i]);
  return (uint32_t)wl_block_fold<WlMax>(best);
}

// Round `sample`, before its walk: the pick (every workgroup by itself: it waits for nobody) and the work list.
__global__ __launch_bounds__(WL_BS) void wcc_compact(WccCtl *ctl, int s, WccGraph G, const uint32_t *__restrict__ p,
                                                      uint32_t *__restrict__ list, WlPiece *__restrict__ ipieces, WlPiece *__restrict__ opieces) {
  if (ctl->step != s || s != ctl->sample) return;
  const uint32_t L = s > 0 ? wcc_pick(p, G.rows) : WCC_NONE;
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool walk = v < G.rows && p[v] != L;
    const uint32_t at = wl_wave_append(&ctl->n, walk, lane);
    if (walk) {   // (only this lane looks at v, and only in this launch: invariant 1)
      list[at] = (uint32_t)v;
      wl_push_pieces<WCC_PIECE>(&ctl->nip, (uint32_t)v, (uint32_t)(G.in_ptr[v + 1] - G.in_ptr[v]), ipieces);
      wl_push_pieces<WCC_PIECE>(&ctl->nop, (uint32_t)v, (uint32_t)(G.out_ptr[v + 1] - G.out_ptr[v]), opieces);
    }
  }
}

// A full round's walk: the in-lists and the out-lists of the work list's vertices, a hook per entry.
__global__ __launch_bounds__(WL_BS) void wcc_full(const WccCtl *ctl, int s, WccGraph G, uint32_t *p, const uint32_t *__restrict__ list,
                                                   const WlPiece *__restrict__ ipieces, const WlPiece *__restrict__ opieces,
                                                   WlPart *__restrict__ part) {
  if (ctl->step != s || s < ctl->sample) return;
  uint32_t hooks = 0, open = 0;
  const auto self = [](int32_t v, bool) { return (uint32_t)v; };
  const auto tally = [&](int r) { hooks += r == 1; open += r != 0; };
  const int64_t n = ctl->n;
  uint32_t looked = wl_expand<WCC_SHORT, WCC_PIECE>(list, n, ipieces, ctl->nip, G.in_ptr, self,
                                                    [&](int32_t j, uint32_t v) { tally(wcc_hook(p, (uint32_t)G.in_col[j], v)); });
  looked += wl_expand<WCC_SHORT, WCC_PIECE>(list, n, opieces, ctl->nop, G.out_ptr, self,
                                            [&](int32_t j, uint32_t v) { tally(wcc_hook(p, v, (uint32_t)G.out_row[j])); });
  wl_block_part<WlSum, WlSum>(part, looked, hooks, open);
}

// Jumping launch i of round s, over all rows: wl_jump, WCC_JUMPS jumps per vertex at most.
__global__ __launch_bounds__(WL_BS) void wcc_jump(WccCtl *ctl, int s, int i, int32_t rows, uint32_t *p, WlPart *__restrict__ jpart) {
  if (ctl->step != s || (i > 0 && !ctl->moved[i - 1])) return;
  wl_jump(i, WCC_JUMPS, rows, p, jpart, ctl->moved);
}

// Closes round s (slot k of the batch).  One workgroup sums the WlParts (no atomics on one word: they retire about 6 ns
// apart, see frontier_detect) and its first lane records the round and decides.
__global__ __launch_bounds__(WL_BS) void wcc_decide(WccCtl *ctl, int k, int s, int nparts, const WlPart *__restrict__ part,
                                                     const WlPart *__restrict__ jpart) {
  if (!wl_from_thread0(ctl->step == s)) return;
  uint32_t t[4] = {0u, 0u, 0u, 0u};   // entries looked at, hooks, entries left unsettled, pointers changed
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) { t[0] += part[i].a; t[1] += part[i].b; t[2] += part[i].c; t[3] += jpart[i].a; }
  for (int f = 0; f < 4; f++) t[f] = wl_block_fold<WlSum>(t[f]);
  if (threadIdx.x != 0) return;
  const bool full = s >= ctl->sample;
  if (s == ctl->sample) ctl->skipped = ctl->rows - ctl->n;
  ctl->rec[k] = WccRec{1, full ? WCC_KIND_FULL : WCC_KIND_SAMPLE, t[1], t[3], t[0]};
  for (int i = 0; i < WCC_SWEEPS; i++) ctl->moved[i] = 0u;
  if (full && t[2] == 0u && t[3] == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = s + 1;
}

// Closes the call: comp[v] = p[v], or -1 everywhere after an incomplete run (a half-built forest is no partition), and
// the number of roots.
__global__ __launch_bounds__(WL_BS) void wcc_label(WccCtl *ctl, int32_t rows, int complete, const uint32_t *__restrict__ p,
                                                    int32_t *__restrict__ comp) {
  uint32_t roots = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    const uint32_t up = p[v];
    comp[v] = complete ? (int32_t)up : -1;
    roots += (complete && up == (uint32_t)v) ? 1u : 0u;
  }
  roots = wl_block_fold<WlSum>(roots);
  if (threadIdx.x == 0 && roots) wl_add(&ctl->components, roots);   // (one add per workgroup)
}

} // namespace sh
