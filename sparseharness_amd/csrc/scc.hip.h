// scc.hip.h -- kernels of sh_scc: strongly connected components by trimming, one pivot round and colouring rounds
// (forward-backward with trim: Fleischer, Hendrickson, Pinar, "On identifying strongly connected components in parallel",
// IPDPS 2000 workshops; colouring: Orzan, "On distributed verification and verified distribution", 2004; their mix on
// shared memory: Slota, Rajamanickam, Madduri, "BFS and coloring-based parallel algorithms for strongly connected
// components and related problems", IPDPS 2014).  comp[v] becomes the largest vertex index of v's component
// (DESIGN.md "6g Strongly connected components").
//
// The graph lives in the layout of sh_bfs_graph (in_ptr / in_col: the edges c -> r by row r; out_ptr / out_row: by source
// vertex c).  A vertex is LIVE while comp[v] == -1; edges count only between live vertices and self-loops never count.
// A STEP is one sweep, and every sweep belongs to a phase of the state machine in SccCtl:
//   TRIM   scc_trim    sweep 0 looks at every live vertex: one with no live in-neighbour or no live out-neighbour is a
//                      component of its own (the search through a list stops at its first live neighbour, as
//                      bfs_bottomup's does).  Later sweeps look only at the neighbours of what the sweep before settled.
//   SEED   scc_pick + scc_seed   open a round.  Pivot round: p = the live vertex with the largest (in-list length) x
//                      (out-list length), ties to the largest index, by per-workgroup partials; colour = 1 at p, 0
//                      elsewhere; list = {p}.  Colouring round: colour[v] = v and all live vertices on the list.
//   PROP   scc_propagate   the list's vertices push their colour along their out-lists by atomic max; the lane that
//                      raised colour[r] files r for the next sweep.  Ends when a sweep files nothing: colour[u] is then
//                      the largest live index that reaches u (pivot round: 1 iff p reaches u).
//   CLAIM  scc_claim   sweep 0 claims the roots (colouring: every live v with colour[v] == v, comp[v] = v; pivot: p).
//                      Later sweeps walk the in-lists of what the sweep before claimed and claim every live c whose
//                      colour is that of the claimed vertex it has an edge to (colouring: comp[c] = the colour, final at
//                      once; pivot: colour 1 -> 2, the largest claimed index is carried along in the WlParts).
//   LABEL  scc_label   closes the pivot round: comp[c] = the largest claimed index for every claimed c.
// scc_decide closes every step: it sums the WlParts, records the step and moves the state machine.
//
// Invariant 1: NO LIST CAN OVERFLOW ON ANY INPUT.  A vertex is appended
//   - to a list of settled vertices (trim) when it is settled: once per call, by the one lane that looks at it (sweep 0
//     looks at every row once; later sweeps look at the candidate list, see next line);
//   - to the candidate list (trim) or to the next propagation list at most once per sweep: only the lane that raises
//     stamp[r] to the sweep's tag (the step number plus one; it only grows, by atomic max) appends;
//   - to a list of claimed vertices when it is claimed: once per round, by the lane that wins a compare-and-swap.
// Lists of `rows` entries therefore suffice, and each piece list is bounded by edges / 1024 + 1 (wl_push_pieces).
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE.  There is no spin loop and no handshake between
// workgroups inside a launch; every loop is bounded by a length read once at its start; the gate words a kernel reads
// were written by a launch that ended before it.  Values are written with vector stores or plain C++ only.  Lanes of
// one sweep do race on comp / colour, in one direction only (a live vertex is settled, a colour grows): a stale word
// costs a later sweep, never a wrong answer.  max_steps bounds the call.
//
// Work distribution as worklist.hip.h describes it.  The handle is built by its kernels (wl_edge_flag<BfsKeep>, ...).
#pragma once
#include "bfs.hip.h"
#include "worklist.hip.h"

namespace sh {

constexpr int SCC_SHORT = 8;             // lists up to this many edges: one lane each (pushes)
constexpr int SCC_TRIM_SHORT = 32;       // trim: lists up to this many edges one lane each (the early exit keeps a lane's walk short)
constexpr int SCC_PIECE = 2048;          // lists above this are walked in pieces of this many edges
constexpr int SCC_ROW_PIECE = 4096;      // the shared builder's static row pieces (the search does not use them)
constexpr int SCC_BATCH = 32;            // steps enqueued ahead of the host at most (the first batch holds 8)
constexpr int SCC_MAX_BLOCKS = 1024;     // workgroups of a launch at most: one WlPart and one SccPick each
constexpr int SCC_CTL_BYTES = 2048;      // device bytes set aside for SccCtl
constexpr int SCC_PART_BYTES = 16 * SCC_MAX_BLOCKS;
constexpr int SCC_PICK_BYTES = 16 * SCC_MAX_BLOCKS;

enum : int32_t { SCC_TRIM = 0, SCC_SEED = 1, SCC_PROP = 2, SCC_CLAIM = 3, SCC_LABEL = 4 };   // SccCtl::phase
enum : int32_t { SCC_KIND_TRIM = 0, SCC_KIND_PIVOT = 1, SCC_KIND_COLOUR = 2 };               // kind_per_round

struct SccRec {   // what step k of a batch did (read back by the host once per batch)
  int32_t ran, kind, round;   // round: which run of steps it belongs to (the host adds the steps of one round up)
  uint32_t settled, edges;
};
struct SccPick {  // a workgroup's candidate for the pivot
  uint64_t prod;
  int32_t v, pad;
};
// Control block in device memory.  The list a sweep reads is list `cur` (with the pieces of its long out- and in-lists),
// the one it fills is the other.
struct SccCtl {
  uint32_t n[2], nop[2], nip[2];    // length of list 0 / 1, of its out-list pieces, of its in-list pieces
  uint32_t ncand;                   // length of the trim's candidate list
  int32_t step;                     // the step that runs next (-1 once the run has finished)
  int32_t phase, kind, sweep;       // its phase; the kind of the round it belongs to; its number inside the phase
  int32_t cur;
  int32_t finished;
  int32_t opt_trim, opt_pivot;      // the caller's settings
  int32_t pivot_done, pivot, pmax;  // the pivot round has run; its vertex; the largest index claimed so far
  int32_t round;                    // the run of steps that is open
  uint32_t rows, settled, trimmed, components;
  SccRec rec[SCC_BATCH];
};
// The WlPart of a workgroup: a = edges looked at, b = vertices settled / claimed / labelled, c = the largest claimed
// index plus one (pivot round).

struct SccGraph {   // the handle's edge lists, as a kernel argument
  int32_t rows;
  const int32_t *in_ptr, *in_col, *out_ptr, *out_row;
};
struct SccLists {   // the handle's work lists, as a kernel argument
  uint32_t *l0, *l1, *cand;
  WlPiece *op0, *op1, *ip0, *ip1;
  __device__ uint32_t *list(int i) const { return i ? l1 : l0; }
  __device__ WlPiece *op(int i) const { return i ? op1 : op0; }
  __device__ WlPiece *ip(int i) const { return i ? ip1 : ip0; }
};

__device__ __forceinline__ bool scc_cas(int32_t *p, int32_t expect, int32_t v) {
  return __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// v takes place `at` of list q; the pieces of its long out- and in-list join the list's piece lists
__device__ __forceinline__ void scc_file(SccCtl *ctl, const SccGraph &G, const SccLists &L, int q, uint32_t at, uint32_t v) {
  L.list(q)[at] = v;
  wl_push_pieces<SCC_PIECE>(&ctl->nop[q], v, (uint32_t)(G.out_ptr[v + 1] - G.out_ptr[v]), L.op(q));
  wl_push_pieces<SCC_PIECE>(&ctl->nip[q], v, (uint32_t)(G.in_ptr[v + 1] - G.in_ptr[v]), L.ip(q));
}

// Is pivot candidate a (product, vertex; v < 0: none) better than b?  The larger product, ties to the larger index.
__device__ __forceinline__ bool scc_better(uint64_t pa, int32_t va, uint64_t pb, int32_t vb) {
  return va >= 0 && (vb < 0 || pa > pb || (pa == pb && va > vb));
}
// The workgroup's best pivot candidate -> every thread (convergent control flow only): shuffles inside a wave, one
// shared word pair per wave.  It stays beside wl_block_fold: that folds one word, this an arg-max over a pair whose two
// halves must travel together.  One call per kernel (its words have no barrier ahead of them).
__device__ __forceinline__ void scc_block_best(uint64_t *best, int32_t *bv) {
  __shared__ uint64_t s_prod[WL_BS / 64];
  __shared__ int32_t s_v[WL_BS / 64];
  uint64_t b = *best;
  int32_t v = *bv;
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(b >> 32), o);
    const int32_t ov = __shfl_xor(v, o);
    const uint64_t ob = ((uint64_t)hi << 32) | lo;
    if (scc_better(ob, ov, b, v)) { b = ob; v = ov; }
  }
  if (wl_lane() == 0) { s_prod[threadIdx.x >> 6] = b; s_v[threadIdx.x >> 6] = v; }
  __syncthreads();
  b = s_prod[0]; v = s_v[0];
  for (int w = 1; w < WL_BS / 64; w++)
    if (scc_better(s_prod[w], s_v[w], b, v)) { b = s_prod[w]; v = s_v[w]; }
  *best = b; *bv = v;
}

// comp = -1 (every vertex live) and stamp = 0, for every row
__global__ __launch_bounds__(WL_BS) void scc_init(int32_t rows, int32_t *__restrict__ comp, uint32_t *__restrict__ stamp) {
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    comp[v] = -1;
    stamp[v] = 0u;
  }
}

// Has v (where `on`) a live neighbour other than itself in adj[ptr[v], ptr[v + 1])?  Lists up to SCC_TRIM_SHORT one lane
// each, longer ones the whole wave, 64 entries at a time; both stop at the first hit.  All lanes of the wave call it.
// A long list is NOT cut into pieces here: the search is sequential by nature (it ends at the first live neighbour), and
// on a list whose front is live it reads one group.  Its worst case is a hub all of whose neighbours are settled: one
// wave then reads the whole list, len / 64 dependent groups (a list of a million entries: 16 384 groups, of the order
// of ten milliseconds), once per sweep in which the hub is a candidate, and the sweep waits for that wave.
__device__ __forceinline__ bool scc_any_live(const int32_t *__restrict__ ptr, const int32_t *__restrict__ adj, const int32_t *comp,
                                             int32_t v, bool on, uint32_t *looked) {
  const int lane = wl_lane();
  const int32_t s = on ? ptr[v] : 0;
  const int32_t len = on ? ptr[v + 1] - s : 0;
  bool hit = false;
  if (len <= SCC_TRIM_SHORT)
    for (int32_t j = 0; j < len; j++) {
      (*looked)++;
      const int32_t u = adj[s + j];
      if (u != v && comp[u] == -1) { hit = true; break; }   // the early exit
    }
  uint64_t m = __ballot(len > SCC_TRIM_SHORT);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int32_t sb = __shfl(s, src), lb = __shfl(len, src), vb = __shfl(v, src);
    bool h = false;
    uint32_t seen = 0;
    for (int32_t j0 = 0; j0 < lb; j0 += 64) {
      bool mine = false;
      if (j0 + lane < lb) {
        const int32_t u = adj[sb + j0 + lane];
        mine = u != vb && comp[u] == -1;
      }
      seen += (uint32_t)min(64, lb - j0);
      if (__ballot(mine)) { h = true; break; }
    }
    if (lane == src) { hit = h; *looked += seen; }
  }
  return hit;
}

// A trim sweep, two launches.  Phase 0 (not in sweep 0): the live neighbours of what the sweep before settled become the
// candidates, each once (stamp).  Phase 1: every candidate (sweep 0: every row) that is live and has no live
// in-neighbour or no live out-neighbour is settled as its own component and joins the next list.
__global__ __launch_bounds__(WL_BS) void scc_trim(SccCtl *ctl, int s, int phase, SccGraph G, SccLists L, int32_t *comp, uint32_t *stamp,
                                                   WlPart *part) {
  if (ctl->step != s || ctl->phase != SCC_TRIM) return;
  const int sweep = ctl->sweep, p = ctl->cur, q = p ^ 1, lane = wl_lane();
  if (phase == 0) {
    if (sweep == 0) return;
    const uint32_t tag = (uint32_t)s + 1u;
    const auto file = [&](int32_t r) {
      if (comp[r] == -1 && wl_umax(&stamp[r], tag) < tag) L.cand[wl_append_here(&ctl->ncand)] = (uint32_t)r;
    };
    const auto none = [](int32_t, bool) { return 0u; };
    const int64_t n = ctl->n[p];
    uint32_t looked = wl_expand<SCC_SHORT, SCC_PIECE>(L.list(p), n, L.op(p), ctl->nop[p], G.out_ptr, none,
                                                      [&](int32_t j, uint32_t) { file(G.out_row[j]); });
    looked += wl_expand<SCC_SHORT, SCC_PIECE>(L.list(p), n, L.ip(p), ctl->nip[p], G.in_ptr, none,
                                              [&](int32_t j, uint32_t) { file(G.in_col[j]); });
    wl_block_part(part, looked, 0u);
    return;
  }
  uint32_t looked = (threadIdx.x == 0 && sweep > 0) ? part[blockIdx.x].a : 0u;   // (what phase 0 of this workgroup looked at)
  uint32_t settled = 0;
  const int64_t n = sweep == 0 ? (int64_t)G.rows : (int64_t)ctl->ncand;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const int32_t v = !valid ? 0 : sweep == 0 ? (int32_t)(base + lane) : (int32_t)L.cand[base + lane];
    const bool on = valid && comp[v] == -1;
    const bool has_in = scc_any_live(G.in_ptr, G.in_col, comp, v, on, &looked);
    const bool has_out = scc_any_live(G.out_ptr, G.out_row, comp, v, on && has_in, &looked);
    const bool die = on && !(has_in && has_out);
    const uint32_t at = wl_wave_append(&ctl->n[q], die, lane);
    if (die) {
      comp[v] = v;   // (only this lane looks at v in this sweep)
      scc_file(ctl, G, L, q, at, (uint32_t)v);
      settled++;
    }
  }
  wl_block_part(part, looked, settled);   // (thread 0 alone read the phase-0 word, and it alone replaces it)
}

// The pivot round's candidate of every workgroup: the live vertex with the largest (in-list length) x (out-list length)
// as uint64, ties to the largest index (v = -1: the workgroup saw no live vertex).
__global__ __launch_bounds__(WL_BS) void scc_pick(const SccCtl *ctl, int s, SccGraph G, const int32_t *__restrict__ comp,
                                                   SccPick *__restrict__ pick) {
  if (ctl->step != s || ctl->phase != SCC_SEED || ctl->kind != SCC_KIND_PIVOT) return;
  uint64_t best = 0;
  int32_t bv = -1;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < G.rows; v += (int64_t)gridDim.x * WL_BS) {   // (v ascends)
    if (comp[v] != -1) continue;
    const uint64_t prod = (uint64_t)(uint32_t)(G.in_ptr[v + 1] - G.in_ptr[v]) * (uint64_t)(uint32_t)(G.out_ptr[v + 1] - G.out_ptr[v]);
    if (bv < 0 || prod >= best) { best = prod; bv = (int32_t)v; }
  }
  scc_block_best(&best, &bv);
  if (threadIdx.x == 0) pick[blockIdx.x] = SccPick{best, bv, 0};
}

// Opens a round: the colours and the first list.  Pivot round: every workgroup reduces the candidates of scc_pick by
// itself (at most 1024 out of L2) and so knows p without waiting for anybody.
__global__ __launch_bounds__(WL_BS) void scc_seed(SccCtl *ctl, int s, int nparts, SccGraph G, SccLists L, const int32_t *__restrict__ comp,
                                                   uint32_t *__restrict__ colour, const SccPick *__restrict__ pick) {
  if (ctl->step != s || ctl->phase != SCC_SEED) return;
  const int q = ctl->cur ^ 1, lane = wl_lane();
  if (ctl->kind == SCC_KIND_PIVOT) {
    uint64_t best = 0;
    int32_t p = -1;
    for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) {
      const SccPick c = pick[i];
      if (scc_better(c.prod, c.v, best, p)) { best = c.prod; p = c.v; }
    }
    scc_block_best(&best, &p);
    for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < G.rows; v += (int64_t)gridDim.x * WL_BS)
      colour[v] = v == p ? 1u : 0u;   // (every word: a settled vertex may hold anything from an earlier call)
    if (blockIdx.x == 0 && threadIdx.x == 0 && p >= 0) {
      ctl->pivot = p;   // (read by scc_claim, not in this launch)
      scc_file(ctl, G, L, q, wl_add(&ctl->n[q], 1u), (uint32_t)p);
    }
    return;
  }
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool live = v < G.rows && comp[v] == -1;
    if (live) colour[v] = (uint32_t)v;
    const uint32_t at = wl_wave_append(&ctl->n[q], live, lane);
    if (live) scc_file(ctl, G, L, q, at, (uint32_t)v);
  }
}

// A propagation sweep: colour[r] = max(colour[r], colour[v]) along every edge v -> r between live vertices, v from the
// list.  The lane that raised the word files r, at most once per sweep (stamp): see invariant 1.
__global__ __launch_bounds__(WL_BS) void scc_propagate(SccCtl *ctl, int s, SccGraph G, SccLists L, const int32_t *__restrict__ comp,
                                                        uint32_t *colour, uint32_t *stamp, WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->phase != SCC_PROP) return;
  const int p = ctl->cur, q = p ^ 1;
  const uint32_t tag = (uint32_t)s + 1u;
  const uint32_t looked = wl_expand<SCC_SHORT, SCC_PIECE>(
      L.list(p), ctl->n[p], L.op(p), ctl->nop[p], G.out_ptr, [&](int32_t v, bool) { return colour[v]; },
      [&](int32_t j, uint32_t c) {
        const int32_t r = G.out_row[j];
        if (comp[r] != -1 || colour[r] >= c) return;   // (a stale colour is a smaller one: this never skips a raise)
        if (wl_umax(&colour[r], c) < c && wl_umax(&stamp[r], tag) < tag)
          scc_file(ctl, G, L, q, wl_append_here(&ctl->n[q]), (uint32_t)r);
      });
  wl_block_part(part, looked, 0u);
}

// A claim sweep.  Sweep 0 claims the roots; later sweeps walk the in-lists of what the sweep before claimed.
__global__ __launch_bounds__(WL_BS) void scc_claim(SccCtl *ctl, int s, SccGraph G, SccLists L, int32_t *comp, uint32_t *colour,
                                                    WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->phase != SCC_CLAIM) return;
  const int p = ctl->cur, q = p ^ 1, lane = wl_lane();
  const bool pivot = ctl->kind == SCC_KIND_PIVOT;
  uint32_t looked = 0, claimed = 0, top = 0;
  if (ctl->sweep == 0) {
    if (pivot) {
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t v = ctl->pivot;
        colour[v] = 2u;
        scc_file(ctl, G, L, q, wl_add(&ctl->n[q], 1u), (uint32_t)v);
        claimed = 1; top = (uint32_t)v + 1u;
      }
    } else {
      for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
        const int64_t v = base + lane;
        const bool root = v < G.rows && comp[v] == -1 && colour[v] == (uint32_t)v;
        const uint32_t at = wl_wave_append(&ctl->n[q], root, lane);
        if (root) {
          comp[v] = (int32_t)v;   // (only this lane looks at v in this sweep)
          scc_file(ctl, G, L, q, at, (uint32_t)v);
          claimed++;
        }
      }
    }
  } else {
    looked = wl_expand<SCC_SHORT, SCC_PIECE>(
        L.list(p), ctl->n[p], L.ip(p), ctl->nip[p], G.in_ptr, [&](int32_t v, bool) { return pivot ? 1u : colour[v]; },
        [&](int32_t j, uint32_t k) {
          const int32_t c = G.in_col[j];
          if (colour[c] != k || comp[c] != -1) return;   // (the colour of a settled vertex is stale: it must be live)
          if (pivot ? !scc_cas((int32_t *)&colour[c], 1, 2) : !scc_cas(&comp[c], -1, (int32_t)k)) return;
          scc_file(ctl, G, L, q, wl_append_here(&ctl->n[q]), (uint32_t)c);
          claimed++;
          top = max(top, (uint32_t)c + 1u);
        });
  }
  wl_block_part<WlSum, WlMax>(part, looked, claimed, top);
}

// Closes the pivot round: what it claimed (live, colour 2) gets the largest claimed index as its label.
__global__ __launch_bounds__(WL_BS) void scc_label(const SccCtl *ctl, int s, int32_t rows, int32_t *__restrict__ comp,
                                                    const uint32_t *__restrict__ colour, WlPart *__restrict__ part) {
  if (ctl->step != s || ctl->phase != SCC_LABEL) return;
  const int32_t label = ctl->pmax;
  uint32_t n = 0;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS)
    if (comp[v] == -1 && colour[v] == 2u) { comp[v] = label; n++; }
  wl_block_part(part, 0u, n);
}

// What follows a round that left live vertices behind: a trim round after a pivot or colouring round (when the caller
// trims), else the pivot round (once per call, when the caller wants it), else a colouring round.
__device__ __forceinline__ void scc_next_round(SccCtl *ctl, bool after_trim) {
  ctl->sweep = 0;
  if (ctl->opt_trim && !after_trim) { ctl->phase = SCC_TRIM; ctl->kind = SCC_KIND_TRIM; return; }
  ctl->phase = SCC_SEED;
  ctl->kind = (ctl->opt_pivot && !ctl->pivot_done) ? SCC_KIND_PIVOT : SCC_KIND_COLOUR;
  ctl->pmax = -1;
}

// Closes step s (slot k of the batch); s = -1 closes scc_init.  One workgroup sums the WlParts (no atomics on one word:
// they retire about 6 ns apart, see frontier_detect) and its first lane moves the state machine.
__global__ __launch_bounds__(WL_BS) void scc_decide(SccCtl *ctl, int k, int s, int nparts, const WlPart *__restrict__ part, int32_t rows,
                                                     int32_t trim, int32_t pivot) {
  if (!wl_from_thread0(s < 0 || ctl->step == s)) return;
  if (s < 0) {
    if (threadIdx.x != 0) return;
    ctl->rows = (uint32_t)rows; ctl->opt_trim = trim; ctl->opt_pivot = pivot;
    scc_next_round(ctl, false);
    ctl->step = 0;
    return;
  }
  const WlPart sums = wl_sum_parts<WlSum, WlMax>(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t a = sums.a, b = sums.b, c = sums.c;
  const int ph = ctl->phase, p = ctl->cur, kind = ctl->kind;
  uint32_t settled = 0, edges = 0;
  bool round_end = false;
  if (ph != SCC_LABEL) {   // the list the sweep read is done with; the one it filled is the next sweep's
    ctl->n[p] = 0; ctl->nop[p] = 0; ctl->nip[p] = 0;
    ctl->cur = p ^ 1;
  }
  const bool more = ctl->n[p ^ 1] > 0;
  if (ph == SCC_TRIM) {
    settled = b; edges = a;
    ctl->trimmed += b; ctl->components += b;
    ctl->ncand = 0;
    round_end = !more;
  } else if (ph == SCC_SEED) {
    ctl->phase = SCC_PROP;
  } else if (ph == SCC_PROP) {
    edges = a;
    if (!more) ctl->phase = SCC_CLAIM;
  } else if (ph == SCC_CLAIM) {
    edges = a;
    if (kind == SCC_KIND_COLOUR) {
      settled = b;
      if (ctl->sweep == 0) ctl->components += b;   // the roots
    } else {
      ctl->pmax = max(ctl->pmax, (int32_t)c - 1);
    }
    if (!more) {
      if (kind == SCC_KIND_PIVOT) ctl->phase = SCC_LABEL;
      else round_end = true;
    }
  } else {
    settled = b;
    ctl->components += 1u;
    ctl->pivot_done = 1;
    round_end = true;
  }
  ctl->sweep = (ctl->phase == ph) ? ctl->sweep + 1 : 0;
  ctl->settled += settled;
  ctl->rec[k] = SccRec{1, kind, ctl->round, settled, edges};
  if (round_end || ctl->settled == ctl->rows) {
    ctl->round++;
    if (ctl->settled == ctl->rows) { ctl->finished = 1; ctl->step = -1; return; }
    scc_next_round(ctl, ph == SCC_TRIM);
  }
  ctl->step = s + 1;
}

} // namespace sh
