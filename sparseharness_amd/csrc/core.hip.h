// core.hip.h -- kernels of sh_core: the core number of every vertex (k-core decomposition) by parallel peeling, level by
// level (the peeling order: Matula, Beck, "Smallest-last ordering and clustering and graph coloring algorithms", J. ACM
// 1983; the bucket algorithm of the host gold: Batagelj, Zaversnik, "An O(m) algorithm for cores decomposition of
// networks", 2003; peeling a level in parallel rounds with atomic decrements: Dhulipala, Blelloch, Shun, "Julienne",
// SPAA 2017).  core[v] is the largest k such that v lies in a subgraph whose vertices all have at least k neighbours in
// it (DESIGN.md "6j k-core decomposition").
//
// The graph is sh_tri's simple undirected graph, kept as symmetric lists: ptr[rows + 1] / col[2M], every list strictly
// ascending, deg[v] = ptr[v + 1] - ptr[v].  The state of a call is cur[v], the REMAINING DEGREE of v, and core[v], -1
// until v is SETTLED.  A call walks the levels k upwards; inside a level it runs ROUNDS.  The invariant at the start of
// every round: the current work list holds exactly the unsettled vertices with cur[v] <= k, each once, and for every
// unsettled vertex outside it cur[v] > k is the number of its unsettled neighbours.  A round is one step of the control
// block, a fixed set of launches:
//   core_min    only when the round OPENS A LEVEL (the work list is empty and vertices remain): the smallest cur[v] among
//               the unsettled, per workgroup, into one word per workgroup (not one word hit by every wave).
//   core_open   same gate: k = the smallest of those words (every workgroup folds them by itself: it waits for nobody),
//               so empty levels are skipped, not walked; every unsettled v with cur[v] <= k joins the work list and the
//               pieces of a list above CORE_PIECE entries join the piece list.
//   core_peel   wl_expand<CORE_SHORT, CORE_PIECE> over the work list: the visit settles v (core[v] = k); every entry u
//               with cur[u] > k gets ONE atomic decrement.  The one lane that sees the old value k + 1 OWNS u: it appends
//               u to the next list (with its pieces) or chases it (below).  A lane that sees an old value <= k restores
//               it with one add.  No compare-and-swap, no retry.
//   core_close  one workgroup: sums the WlParts, takes the settled vertices from `remaining`, empties the list just
//               walked, swaps the lists, records the round, decides whether the next round opens a level, and finishes
//               when nothing remains.
//
// The decrement, and why TRANSIENT VALUES BELOW k ARE HARMLESS.  Take a vertex u with cur[u] = c > k when a round of level
// k starts, and let d lanes of the round reach the atomic decrement of cur[u].  Order the atomics on the word as memory
// does.  (1) While the word is > k + 1 a decrement returns an old value > k + 1 and is final.  (2) The decrement that
// returns exactly k + 1 leaves k.  From then on the word is k minus the number of decrements that returned <= k and
// have not restored yet: a decrement takes it one lower and is followed by that same lane's add of one, and no other
// operation touches it.  So the word never exceeds k again: (3) AT MOST ONE decrement of the call returns k + 1 for u --
// the owner is unique -- and exactly one does if d >= c - k.  (4) Every reader only asks `> k`: a transient k - 1, k - 2,
// ... answers like k, "u is owned already", which is true; a stale larger word leads to a decrement, which memory
// orders as above.  (5) When the launch has ended every restore has landed: cur[u] = max(k, c - d).  A signed word is
// used, so a transient below zero at k = 0 is as harmless.  The set owned in a round therefore depends on the graph and
// the round's work list alone, not on the schedule.
//
// CHASE (chase > 0).  A lane that owns a u whose list has at most CORE_SHORT entries keeps it in hand instead of
// appending it -- at most one; any other it comes to own goes to the next list.  When wl_expand has returned, the lane
// settles the u in hand (core[u] = k) and walks u's list with the same decrement, which may put another vertex in its
// hand; that at most `chase` times in a row; what it still holds then goes to the next list.  A chain hanging off the
// level's vertices (a path, a tree's branch) is thereby eaten chase + 1 vertices per end and round, not one: a path of n
// vertices takes about n / (2 (chase + 1)) rounds instead of n / 2.
//
// Why the core numbers do not depend on `chase`, the schedule or the run, and why chasing never costs a round.
// PEELING IS MONOTONE: settling more vertices only lowers remaining degrees further.  Level k ends when no unsettled
// vertex has cur <= k; the vertices settled in it are the closure "delete every vertex of remaining degree <= k until
// none is left", which is the same set in whatever order and grouping the deletions happen, and cur of the others is
// then their degree in what is left (each settled neighbour took exactly one, see (1)).  So every level starts from one
// state under every schedule, and core[v] = the level v fell in.  Rounds: let A be the settled set of a chasing run and
// B that of the run with chase == 0 after the same number of rounds, same level, A containing B.  A vertex of remaining
// degree <= k after B's deletions has remaining degree <= k after A's; by the invariant it is settled in A or stands in
// A's work list.  One round later A still contains B.  A level that A finishes earlier it also opens earlier.  Hence
// rounds(chase > 0) <= rounds(chase == 0).  With chase == 0 a round's set is exactly the vertices whose remaining degree
// fell to <= k in the round before (or, in an opening round, all with cur == k): rounds, k, size and edges per round are
// deterministic.  With chase > 0 which lane owns what, and so who is chased, depends on the schedule: the records are
// informational; size + chased over all rounds is `rows` either way.
//
// Invariant 1: EVERY VERTEX IS SETTLED ONCE.  A vertex is settled by the visit of a work-list entry or by its chaser.
// It enters a work list either in core_open -- by the one lane that looks at it, and only while it is unsettled and in
// no list, because core_open runs only when the list is empty, and every owned vertex has been appended or chased by
// then -- or by its owner, which is unique by (3) and either appends it or chases it, never both.  A vertex core_open
// lists has cur <= k and is never owned afterwards (owning needs an old value k' + 1 > k at a later level, but it is
// settled in this round).  So a list of `rows` places cannot overflow, a piece list is bounded by 2M / (CORE_PIECE / 2) + 1
// (wl_push_pieces), and `remaining` reaches zero exactly when every vertex is settled.
// Invariant 2: NO KERNEL EVER WAITS for another kernel's write, and no lane for another lane's.  There is no spin loop
// and no retry: a decrement is one atomic, a restore one more.  The gate words a launch reads (step, opening, k, p, the
// current list's lengths) were written by a launch that ended before it; what a launch writes to the control block (the
// NEXT list's lengths, core_open's k and the current list's length) no workgroup of that same launch reads as a gate.
// Values are written with vector stores, atomics or plain C++ only.  max_rounds bounds the call.
// Invariant 3: EVERY LOOP IS BOUNDED.  The strided loops by the list length or `rows`; a list walk by the list's length;
// the chase by chase * CORE_SHORT entries per lane (at most `chase` vertices, each of at most CORE_SHORT entries).
//
// Worst cases.  The number of rounds is the depth of the peeling, not the diameter: a path or a grid needs rounds in
// proportion to its side (the 128 x 128 grid: 127 rounds, one level); chase shortens chains of short lists only.  Every
// non-empty level costs two passes over all vertices (core_min, core_open).  A hub's list is walked once, in pieces,
// when the hub is settled; until then every neighbour that goes first pays one atomic on the hub's word.
//
// Work distribution as worklist.hip.h describes it.  The handle is built by its kernels (wl_und_flag<BfsKeep>, ...,
// wl_both_ways, wl_forward_lists).
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int CORE_SHORT = 8;             // lists up to this many entries: one lane each (and the lists a lane chases)
constexpr int CORE_PIECE = 2048;          // lists above this are walked in pieces of this many entries
constexpr int CORE_BATCH = 32;            // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int CORE_MAX_BLOCKS = 1024;     // workgroups of a launch at most: two WlParts each
constexpr int CORE_CTL_BYTES = 2048;      // device bytes set aside for CoreCtl
constexpr int CORE_PART_BYTES = 16 * CORE_MAX_BLOCKS;
constexpr uint32_t CORE_NONE = 0xFFFFFFFFu;   // no unsettled vertex seen (a degree is below 2^31)

struct CoreRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran, k;
  uint32_t size, chased, edges;
};
// Control block in device memory.
struct CoreCtl {
  uint32_t n[2], np[2];          // length of work list 0 / 1, of its piece list
  int32_t p;                     // the list the next round walks (the other one is filled meanwhile)
  int32_t step;                  // the round that runs next (-1 once the run has finished)
  int32_t finished;
  int32_t opening;               // the next round opens a level (its list is empty and vertices remain)
  int32_t k;                     // the level being peeled
  int32_t chase;                 // the caller's setting
  uint32_t remaining;            // unsettled vertices
  int32_t levels, degeneracy;    // levels opened so far, the latest of them
  CoreRec rec[CORE_BATCH];
};
// The WlParts of a workgroup.  core_peel: a = list entries looked at, b = vertices chased.  core_min (an array of its
// own): a = the smallest remaining degree among the workgroup's unsettled vertices, CORE_NONE if it saw none.

struct CoreGraph {   // the handle's lists, as a kernel argument
  int32_t rows;
  const int32_t *ptr, *col;
};
struct CoreLists {   // the two work lists and their piece lists
  uint32_t *list[2];
  WlPiece *pieces[2];
};

// cur = deg, core = -1 for every row; the caller's setting into the control block (which the host has zeroed: step = 0,
// p = 0, both lists empty)
__global__ __launch_bounds__(WL_BS) void core_init(CoreCtl *ctl, int32_t rows, int32_t chase, const uint32_t *__restrict__ deg,
                                                    int32_t *__restrict__ cur, int32_t *__restrict__ core) {
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS) {
    cur[v] = (int32_t)deg[v];
    core[v] = -1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->remaining = (uint32_t)rows; ctl->chase = chase; ctl->opening = 1; }
}

// Opening round s, first pass: the smallest remaining degree among the unsettled, per workgroup.
__global__ __launch_bounds__(WL_BS) void core_min(const CoreCtl *ctl, int s, int32_t rows, const int32_t *__restrict__ cur,
                                                   const int32_t *__restrict__ core, WlPart *__restrict__ mins) {
  if (ctl->step != s || !ctl->opening) return;
  uint32_t best = CORE_NONE;
  for (int64_t v = (int64_t)blockIdx.x * WL_BS + threadIdx.x; v < rows; v += (int64_t)gridDim.x * WL_BS)
    if (core[v] < 0) best = min(best, (uint32_t)cur[v]);
  best = wl_block_fold<WlMin>(best);
  if (threadIdx.x == 0) mins[blockIdx.x] = WlPart{best, 0u, 0u, 0u};
}

// Opening round s, second pass: k and the level's first work list (list p, empty until now).
__global__ __launch_bounds__(WL_BS) void core_open(CoreCtl *ctl, int s, CoreGraph G, const int32_t *__restrict__ cur,
                                                    const int32_t *__restrict__ core, const WlPart *__restrict__ mins, CoreLists L) {
  if (ctl->step != s || !ctl->opening) return;
  uint32_t m = CORE_NONE;
  for (int i = (int)threadIdx.x; i < (int)gridDim.x; i += WL_BS) m = min(m, mins[i].a);
  const int32_t k = (int32_t)wl_block_fold<WlMin>(m);
  const int p = ctl->p;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->k = k;   // (no workgroup of this launch reads it)
  uint32_t *__restrict__ list = L.list[p];
  WlPiece *__restrict__ pieces = L.pieces[p];
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool take = v < G.rows && core[v] < 0 && cur[v] <= k;
    const uint32_t at = wl_wave_append(&ctl->n[p], take, lane);
    if (take) {   // (only this lane looks at v, and v is in no list: invariant 1)
      list[at] = (uint32_t)v;
      wl_push_pieces<CORE_PIECE>(&ctl->np[p], (uint32_t)v, (uint32_t)(G.ptr[v + 1] - G.ptr[v]), pieces);
    }
  }
}

// Round s: settles the work list's vertices and takes one from the remaining degree of their unsettled neighbours.
__global__ __launch_bounds__(WL_BS) void core_peel(CoreCtl *ctl, int s, CoreGraph G, int32_t *cur, int32_t *__restrict__ core,
                                                    CoreLists L, WlPart *__restrict__ part) {
  if (ctl->step != s) return;
  const int32_t k = ctl->k, chase = ctl->chase;
  const int p = ctl->p, q = p ^ 1;
  uint32_t *__restrict__ next = L.list[q];
  WlPiece *__restrict__ npieces = L.pieces[q];
  int32_t held = -1;   // the vertex this lane owns and will chase
  uint32_t chased = 0;
  const auto push = [&](int32_t u, int32_t len) {
    next[wl_append_here(&ctl->n[q])] = (uint32_t)u;
    wl_push_pieces<CORE_PIECE>(&ctl->np[q], (uint32_t)u, (uint32_t)len, npieces);
  };
  const auto hit = [&](int32_t j) {
    const int32_t u = G.col[j];
    if (wl_load(&cur[u]) <= k) return;   // settled, listed or owned
    const int32_t old = __hip_atomic_fetch_add(&cur[u], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == k + 1) {   // this lane owns u
      const int32_t len = G.ptr[u + 1] - G.ptr[u];
      if (chase > 0 && len <= CORE_SHORT && held < 0) held = u;
      else push(u, len);
    } else if (old <= k) {
      (void)__hip_atomic_fetch_add(&cur[u], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  uint32_t looked = wl_expand<CORE_SHORT, CORE_PIECE>(L.list[p], (int64_t)ctl->n[p], L.pieces[p], (int64_t)ctl->np[p], G.ptr,
                                                      [&](int32_t v, bool first) { if (first) core[v] = k; return 0u; },
                                                      [&](int32_t j, uint32_t) { hit(j); });
  for (int32_t c = 0; c < chase && held >= 0; c++) {   // at most chase * CORE_SHORT entries
    const int32_t v = held;
    held = -1;
    core[v] = k;
    chased++;
    const int32_t b = G.ptr[v], e = G.ptr[v + 1];   // e - b <= CORE_SHORT
    looked += (uint32_t)(e - b);
    for (int32_t j = b; j < e; j++) hit(j);
  }
  if (held >= 0) push(held, G.ptr[held + 1] - G.ptr[held]);
  wl_block_part(part, looked, chased);
}

// Closes round s (slot r of the batch).  One workgroup sums the WlParts (no atomics on one word) and its first lane
// records the round and decides.
__global__ __launch_bounds__(WL_BS) void core_close(CoreCtl *ctl, int r, int s, int nparts, const WlPart *__restrict__ part) {
  if (!wl_from_thread0(ctl->step == s)) return;
  const WlPart sums = wl_sum_parts(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t looked = sums.a, chased = sums.b;
  const int p = ctl->p;
  const uint32_t size = ctl->n[p];
  ctl->rec[r] = CoreRec{1, ctl->k, size, chased, looked};
  if (ctl->opening) { ctl->levels++; ctl->degeneracy = ctl->k; }   // (an opened level settles a vertex: k is a core number)
  ctl->remaining -= size + chased;
  ctl->n[p] = 0u; ctl->np[p] = 0u;
  ctl->p = p ^ 1;
  ctl->opening = (ctl->n[p ^ 1] == 0u && ctl->remaining > 0u) ? 1 : 0;
  if (ctl->remaining == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = s + 1;
}

} // namespace sh
