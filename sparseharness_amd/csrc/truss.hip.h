// truss.hip.h -- kernels of sh_truss: the triangles through every edge (its support) and the truss number of every edge
// (k-truss decomposition) by parallel peeling, level by level (the decomposition: Cohen, "Trusses: cohesive subgraphs for
// social network analysis", 2008; the bucket algorithm of the host gold: Wang, Cheng, "Truss decomposition in massive
// networks", VLDB 2012; peeling a level in parallel rounds with atomic decrements and a tie-break by edge id: Kabir,
// Madduri, "Shared-memory graph truss decomposition" (PKT), HiPC 2017).  truss[e] is the largest k such that e lies in a
// subgraph all of whose edges are in at least k - 2 triangles of it; an edge in no triangle has truss 2 (DESIGN.md "6k
// k-truss decomposition").
//
// The graph is sh_tri's simple undirected graph, kept as sh_core's symmetric lists: ptr[rows + 1] / col[2M], every list
// strictly ascending, and next to every list entry the id of its edge, eid[2M].  Edge e, 0 <= e < M, is the e-th smallest
// pair (u, v) with u < v: eu[e], ev[e].  The state of a call, per edge: sup[e], the REMAINING SUPPORT; stamp[e], 0 while
// the edge is alive and in no list, else the round (counted from 1) whose list holds it; truss[e], 0 until e is SETTLED.
// In round r an edge is CURRENT if stamp == r, GONE if 0 < stamp < r, and ALIVE otherwise: 0, or r + 1 (owned during
// this very launch) -- a racing reader sees either of the two and acts the same.  A call walks the levels s upwards
// (k = s + 2); inside a level it runs ROUNDS.  The invariant at the start of every round: the current work list holds
// exactly the unsettled edges with sup[e] <= s, each once, stamped with the round, and for every alive edge outside it
// sup[e] > s is the number of its triangles whose two other edges are not gone.  The launches of a call:
//   truss_init     once: sup = 0, stamp = 0, truss = 0; the edges whose shorter list is above TRUSS_PIECE entries join
//                  the support pass's list of long items.
//   truss_support  once: sup[e] = |N(u) & N(v)| by the walk below; the workgroups' sums into one TrussPart each.
//   truss_total    once, one workgroup: sums them (three per triangle).
// and per round, a step of the control block, a fixed set of launches:
//   truss_min      only when the round OPENS A LEVEL (the work list is empty and edges remain): the smallest sup[e] among
//                  the unsettled, per workgroup, into one word per workgroup (not one word hit by every wave).
//   truss_open     same gate: s = the smallest of those words (every workgroup folds them by itself: it waits for
//                  nobody), so empty levels are skipped, not walked; every unsettled e with sup[e] <= s gets stamp = r
//                  and joins the work list.
//   truss_peel     the walk over the work list: the visit settles e (truss[e] = s + 2); every triangle found goes through
//                  the rule below.
//   truss_close    one workgroup: sums the TrussParts, takes the settled edges from `remaining`, empties the list just
//                  walked, swaps the lists, records the round, decides whether the next round opens a level, and
//                  finishes when nothing remains.
//
// The walk (truss_walk): the item is an edge e = {a, b}, a the end with the shorter list (u on a tie).  Every entry w of
// a's list, with the edge id e1 = {a, w} next to it, is bisected into b's list; a hit gives e2 = {b, w}.  Work goes by
// the length of the shorter list: up to TRUSS_SHORT entries one lane, up to TRUSS_PIECE one wave, longer lists in pieces
// of TRUSS_PIECE entries, one wave per piece.  wl_expand is not used: it takes a list entry as the row whose list it
// walks, here the entry is an edge and carries five words to its lanes; and its piece lists cannot be sized -- an item
// is cut by the SHORTER of two lists, and the sum of those over all edges is not linear in M (K_n: n^2 / 2 edges of
// n / TRUSS_PIECE pieces each).  So a work list keeps its long items at its far end, filled downwards (list[M - 1 - i]),
// and a workgroup takes a long item whole, its waves one piece each in turn: no list of pieces is stored, and the
// handle's footprint stays a closed formula in rows and M.
//
// The rule for a triangle {e, e1, e2} found from current e, and why EVERY TRIANGLE COSTS EACH SURVIVING EDGE ONE DECREMENT:
//   e1 or e2 gone        nothing: the triangle was taken apart in an earlier round, and its survivors paid then.
//   both current         nothing: all three are settled in this round.
//   only e1 current      e2 is decremented if e < e1, else not (and with e1, e2 swapped): the walk from e1 finds the same
//                        triangle with e current, and of the two exactly one acts.
//   neither current      both are decremented: no other walk of this round finds the triangle.
// After round r its current edges are gone for good, so no later round touches the triangle again.  Stamps of r were
// written by a launch that ended before this one; the only stamp written during the launch is r + 1 over 0, both alive.
//
// The decrement is sh_core's, and TRANSIENT VALUES BELOW s ARE HARMLESS for the same reason (core.hip.h has the steps
// (1)-(5), with k read as s): if the word is <= s on a relaxed load, skip; else one atomic -1.  While the word is > s + 1
// a decrement is final.  The one lane that gets the old value s + 1 OWNS the edge: it writes stamp = r + 1 and appends it
// to the next list.  A lane that gets an old value <= s restores it with one add; from the owner's decrement on the word
// is s minus the decrements that have not restored yet and never exceeds s again, so the owner is unique, and every
// reader only asks `> s`.  When the launch has ended, sup[x] = max(s, c - d) for an alive edge that started the round at
// c and lost d triangles.  No compare-and-swap, no retry, no waiting.
//
// Why truss, levels, rounds and the records do not depend on the schedule or the run.  PEELING IS MONOTONE: settling more
// edges only lowers remaining supports further.  Level s ends when no unsettled edge has sup <= s; the edges settled in
// it are the closure "delete every edge of remaining support <= s until none is left", the same set in whatever order
// the deletions happen, and sup of the others is then their support in what is left.  So every level starts from one
// state and truss[e] = the level e fell in, plus 2.  Inside a level a round's list is exactly the edges whose remaining
// support fell to <= s in the round before (or, in an opening round, all with the smallest): rounds, and k, size and
// walked per round are deterministic -- `walked` is the sum of min(deg u, deg v) over the round's list, whatever the
// walk skips.  There is no chase option here.
//
// Invariant 1: EVERY EDGE IS SETTLED ONCE.  An edge is settled by the visit of a work-list entry.  It enters a work list
// either in truss_open -- by the one lane that looks at it, and only while stamp == 0 -- or by its owner, which is
// unique.  An edge truss_open lists has sup <= s and is never owned afterwards.  So the two ends of a list of M places,
// the short items growing upwards and the long ones downwards, cannot meet, and `remaining` reaches zero exactly when
// every edge is settled.
// Invariant 2: NO KERNEL EVER WAITS for another kernel's write, and no lane for another lane's.  There is no spin loop and
// no retry: a decrement is one atomic, a restore one more.  The gate words a launch reads (step, opening, s, p, the
// current list's lengths) were written by a launch that ended before it; what a launch writes to the control block (the
// NEXT list's lengths, truss_open's s and the current list's lengths) no workgroup of that same launch reads as a gate.
// Values are written with vector stores, atomics or plain C++ only.  max_rounds bounds the call.
// Invariant 3: EVERY LOOP IS BOUNDED.  The strided loops by the list lengths or M; a list walk by the list's length; a
// bisection by 32 halvings.
//
// Worst cases.  The number of rounds is the depth of the peeling: the triangulated 128 x 128 grid needs 128 rounds for
// its one level.  Every non-empty level costs two passes over all edges (truss_min, truss_open).  An edge between two
// hubs costs its shorter list, bisected entry by entry into the longer, in the support pass and once more in the round
// in which it is current, by one workgroup.  A clique of n vertices costs n^3 / 2 bisections in the support pass.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int TRUSS_SHORT = 8;             // shorter lists up to this many entries: one lane each
constexpr int TRUSS_PIECE = 2048;          // shorter lists above this are walked in pieces of this many entries
constexpr int TRUSS_BATCH = 32;            // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int TRUSS_MAX_BLOCKS = 1024;     // workgroups of a launch at most
constexpr int TRUSS_CTL_BYTES = 2048;      // device bytes set aside for TrussCtl
constexpr int TRUSS_PART_BYTES = 16 * TRUSS_MAX_BLOCKS;
constexpr uint32_t TRUSS_NONE = 0xFFFFFFFFu;   // no unsettled edge seen (a support is below 2^31)

struct TrussRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran, k;
  uint32_t size, pad;
  uint64_t walked;
};
// Control block in device memory.
struct TrussCtl {
  uint32_t n[2], nl[2];          // work list 0 / 1: its short items (from the front), its long items (from the far end)
  uint32_t nsl;                  // long items of the support pass (at the far end of list 1, which is empty then)
  int32_t p;                     // the list the next round walks (the other one is filled meanwhile)
  int32_t step;                  // the round that runs next, counted from 0 (-1 once the run has finished)
  int32_t finished;
  int32_t opening;               // the next round opens a level (its list is empty and edges remain)
  int32_t s;                     // the level being peeled: k = s + 2
  uint32_t remaining;            // unsettled edges
  int32_t levels, max_truss;     // levels opened so far, the k of the latest of them
  uint64_t hits;                 // the sum of the supports: three per triangle
  TrussRec rec[TRUSS_BATCH];
};
// Per workgroup: truss_support: a = its sum of supports; truss_peel: a = its sum of min(deg u, deg v).  (truss_min's
// words are WlParts: a = the smallest remaining support among the workgroup's unsettled edges, TRUSS_NONE if none.)
struct TrussPart { uint64_t a, pad; };

struct TrussGraph {   // the handle's lists and edges, as a kernel argument
  int32_t rows, edges;
  const int32_t *ptr, *col, *eid, *eu, *ev;
};
struct TrussLists { uint32_t *list[2]; };   // M places each

// Edge e as a work item: a = the end with the shorter list (u on a tie), b the other, [sa, sa + la) a's list.
struct TrussItem { int32_t a, b, sa, la; };
__device__ __forceinline__ TrussItem truss_item(const TrussGraph &G, int32_t e) {
  const int32_t u = G.eu[e], v = G.ev[e];
  const int32_t su = G.ptr[u], lu = G.ptr[u + 1] - su, sv = G.ptr[v], lv = G.ptr[v + 1] - sv;
  return lv < lu ? TrussItem{v, u, sv, lv} : TrussItem{u, v, su, lu};
}
// The entry of w in b's list, or -1 (at most 32 halvings).
__device__ __forceinline__ int32_t truss_find(const TrussGraph &G, int32_t b, int32_t w) {
  int32_t lo = G.ptr[b], hi = G.ptr[b + 1];
  const int32_t end = hi;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (G.col[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < end && G.col[lo] == w) ? lo : -1;
}

// The walk: items [0, n) through item(i) (an edge id, or -1 for a place that holds none; an item whose shorter list is
// above TRUSS_PIECE entries is left to the long items), then the long items far[0], far[-1], ..., far[-(nl - 1)], one
// workgroup each.  visit(e, la) runs once per item; entry(e, b, j) runs once per entry j of the shorter list and returns
// what it counts; done(e, count, shared) gets the count of a lane's item, of a wave's item (lane 0), or of a piece
// (lane 0, shared = true: the item's other pieces report too).
template <class Item, class Visit, class Entry, class Done>
__device__ __forceinline__ void truss_walk(const TrussGraph &G, int64_t n, Item item, const uint32_t *__restrict__ far, int64_t nl,
                                           Visit visit, Entry entry, Done done) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    int32_t e = base + lane < n ? item(base + lane) : -1;
    TrussItem it{0, 0, 0, 0};
    if (e >= 0) {
      it = truss_item(G, e);
      if (it.la > TRUSS_PIECE) { e = -1; it.la = 0; }
    }
    if (e >= 0) visit(e, it.la);
    if (e >= 0 && it.la <= TRUSS_SHORT) {
      uint32_t cnt = 0;
      for (int32_t j = 0; j < it.la; j++) cnt += entry(e, it.b, it.sa + j);
      done(e, cnt, false);
    }
    uint64_t m = __ballot(it.la > TRUSS_SHORT);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t eb = __shfl(e, src), bb = __shfl(it.b, src), sb = __shfl(it.sa, src), lb = __shfl(it.la, src);
      uint32_t cnt = 0;
      for (int32_t j = lane; j < lb; j += 64) cnt += entry(eb, bb, sb + j);
      cnt = wl_wave_sum(cnt);
      if (lane == 0) done(eb, cnt, false);
    }
  }
  for (int64_t h = blockIdx.x; h < nl; h += gridDim.x) {   // a long item: one workgroup, one wave per piece in turn
    const int32_t e = (int32_t)far[-h];
    const TrussItem it = truss_item(G, e);
    if (threadIdx.x == 0) visit(e, it.la);
    for (int32_t off = (int32_t)(threadIdx.x >> 6) * TRUSS_PIECE; off < it.la; off += (WL_BS / 64) * TRUSS_PIECE) {
      const int32_t end = min(off + TRUSS_PIECE, it.la);
      uint32_t cnt = 0;
      for (int32_t j = off + lane; j < end; j += 64) cnt += entry(e, it.b, it.sa + j);
      cnt = wl_wave_sum(cnt);
      if (lane == 0) done(e, cnt, true);
    }
  }
}

// Every edge alive, in no list, its support and its truss number zero; the long items of the support pass.  The caller's
// max_rounds does not come here: the control block was zeroed by the host (step = 0, p = 0, both lists empty).
__global__ __launch_bounds__(WL_BS) void truss_init(TrussCtl *ctl, TrussGraph G, int32_t *__restrict__ sup, int32_t *__restrict__ stamp,
                                                     int32_t *__restrict__ truss, uint32_t *__restrict__ far) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.edges; base += wl_waves() * 64) {
    const int64_t e = base + lane;
    const bool on = e < G.edges;
    if (on) { sup[e] = 0; stamp[e] = 0; truss[e] = 0; }
    const bool heavy = on && truss_item(G, (int32_t)e).la > TRUSS_PIECE;
    const uint32_t at = wl_wave_append(&ctl->nsl, heavy, lane);
    if (heavy) far[-(int64_t)at] = (uint32_t)e;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->remaining = (uint32_t)G.edges; ctl->opening = 1; }
}

// sup[e] = the triangles through e.  A lane's and a wave's item store their count; the pieces of a long item add theirs.
__global__ __launch_bounds__(WL_BS) void truss_support(const TrussCtl *ctl, TrussGraph G, int32_t *sup, const uint32_t *__restrict__ far,
                                                        TrussPart *__restrict__ part) {
  uint64_t total = 0;
  truss_walk(G, (int64_t)G.edges, [](int64_t i) { return (int32_t)i; }, far, (int64_t)ctl->nsl,
             [](int32_t, int32_t) {},
             [&](int32_t, int32_t b, int32_t j) { return truss_find(G, b, G.col[j]) >= 0 ? 1u : 0u; },
             [&](int32_t e, uint32_t cnt, bool shared) {
               total += cnt;
               if (!shared) sup[e] = (int32_t)cnt;
               else if (cnt) (void)__hip_atomic_fetch_add(&sup[e], (int32_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
             });
  total = wl_block_fold<WlSum>(total);
  if (threadIdx.x == 0) part[blockIdx.x] = TrussPart{total, 0ull};
}

__global__ __launch_bounds__(WL_BS) void truss_total(TrussCtl *ctl, int nparts, const TrussPart *__restrict__ part) {
  uint64_t hits = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) hits += part[i].a;
  hits = wl_block_fold<WlSum>(hits);
  if (threadIdx.x == 0) ctl->hits = hits;
}

// Opening round `step`, first pass: the smallest remaining support among the unsettled (with an empty list: those of
// stamp 0), per workgroup.
__global__ __launch_bounds__(WL_BS) void truss_min(const TrussCtl *ctl, int step, int32_t edges, const int32_t *__restrict__ sup,
                                                    const int32_t *__restrict__ stamp, WlPart *__restrict__ mins) {
  if (ctl->step != step || !ctl->opening) return;
  uint32_t best = TRUSS_NONE;
  for (int64_t e = (int64_t)blockIdx.x * WL_BS + threadIdx.x; e < edges; e += (int64_t)gridDim.x * WL_BS)
    if (stamp[e] == 0) best = min(best, (uint32_t)sup[e]);
  best = wl_block_fold<WlMin>(best);
  if (threadIdx.x == 0) mins[blockIdx.x] = WlPart{best, 0u, 0u, 0u};
}

// Opening round `step`, second pass: s and the level's first work list (list p, empty until now).
__global__ __launch_bounds__(WL_BS) void truss_open(TrussCtl *ctl, int step, TrussGraph G, const int32_t *__restrict__ sup,
                                                     int32_t *__restrict__ stamp, const WlPart *__restrict__ mins, TrussLists L) {
  if (ctl->step != step || !ctl->opening) return;
  uint32_t m = TRUSS_NONE;
  for (int i = (int)threadIdx.x; i < (int)gridDim.x; i += WL_BS) m = min(m, mins[i].a);
  const int32_t s = (int32_t)wl_block_fold<WlMin>(m);
  const int p = ctl->p;
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->s = s;   // (no workgroup of this launch reads it)
  uint32_t *__restrict__ list = L.list[p];
  uint32_t *__restrict__ far = list + (G.edges - 1);
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.edges; base += wl_waves() * 64) {
    const int64_t e = base + lane;
    const bool take = e < G.edges && stamp[e] == 0 && sup[e] <= s;
    const bool heavy = take && truss_item(G, (int32_t)e).la > TRUSS_PIECE;
    const uint32_t at = wl_wave_append(&ctl->n[p], take && !heavy, lane);
    const uint32_t atl = wl_wave_append(&ctl->nl[p], heavy, lane);
    if (take) {   // (only this lane looks at e, and e is in no list: invariant 1)
      stamp[e] = step + 1;
      if (heavy) far[-(int64_t)atl] = (uint32_t)e;
      else list[at] = (uint32_t)e;
    }
  }
}

// Round `step`: settles the work list's edges and takes the triangles they close from their surviving edges.
__global__ __launch_bounds__(WL_BS) void truss_peel(TrussCtl *ctl, int step, TrussGraph G, int32_t *sup, int32_t *stamp,
                                                     int32_t *__restrict__ truss, TrussLists L, TrussPart *__restrict__ part) {
  if (ctl->step != step) return;
  const int32_t s = ctl->s, r = step + 1;
  const int p = ctl->p, q = p ^ 1;
  const uint32_t *__restrict__ list = L.list[p];
  uint32_t *__restrict__ next = L.list[q];
  uint32_t *__restrict__ nfar = next + (G.edges - 1);
  uint64_t walked = 0;
  const auto dec = [&](int32_t x) {
    if (wl_load(&sup[x]) <= s) return;   // listed or owned
    const int32_t old = __hip_atomic_fetch_add(&sup[x], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == s + 1) {   // this lane owns x
      __hip_atomic_store(&stamp[x], r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (truss_item(G, x).la > TRUSS_PIECE) nfar[-(int64_t)wl_append_here(&ctl->nl[q])] = (uint32_t)x;
      else next[wl_append_here(&ctl->n[q])] = (uint32_t)x;
    } else if (old <= s) {
      (void)__hip_atomic_fetch_add(&sup[x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  truss_walk(G, (int64_t)ctl->n[p], [&](int64_t i) { return (int32_t)list[i]; }, list + (G.edges - 1), (int64_t)ctl->nl[p],
             [&](int32_t e, int32_t la) { truss[e] = s + 2; walked += (uint64_t)la; },
             [&](int32_t e, int32_t b, int32_t j) {
               const int32_t e1 = G.eid[j];
               const int32_t st1 = wl_load(&stamp[e1]);
               if (st1 > 0 && st1 < r) return 0u;   // gone (no bisection for it)
               const int32_t j2 = truss_find(G, b, G.col[j]);
               if (j2 < 0) return 0u;
               const int32_t e2 = G.eid[j2];
               const int32_t st2 = wl_load(&stamp[e2]);
               if (st2 > 0 && st2 < r) return 0u;
               const bool c1 = st1 == r, c2 = st2 == r;
               if (!c1 && (!c2 || e < e2)) dec(e1);
               if (!c2 && (!c1 || e < e1)) dec(e2);
               return 0u;
             },
             [](int32_t, uint32_t, bool) {});
  walked = wl_block_fold<WlSum>(walked);
  if (threadIdx.x == 0) part[blockIdx.x] = TrussPart{walked, 0ull};
}

// Closes round `step` (slot r of the batch).  One workgroup sums the TrussParts (no atomics on one word) and its first
// lane records the round and decides.
__global__ __launch_bounds__(WL_BS) void truss_close(TrussCtl *ctl, int r, int step, int nparts, const TrussPart *__restrict__ part) {
  if (!wl_from_thread0(ctl->step == step)) return;
  uint64_t walked = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) walked += part[i].a;
  walked = wl_block_fold<WlSum>(walked);
  if (threadIdx.x != 0) return;
  const int p = ctl->p;
  const uint32_t size = ctl->n[p] + ctl->nl[p];
  ctl->rec[r] = TrussRec{1, ctl->s + 2, size, 0u, walked};
  if (ctl->opening) { ctl->levels++; ctl->max_truss = ctl->s + 2; }   // (an opened level settles an edge: k is a truss number)
  ctl->remaining -= size;
  ctl->n[p] = 0u; ctl->nl[p] = 0u;
  ctl->p = p ^ 1;
  ctl->opening = (ctl->n[p ^ 1] + ctl->nl[p ^ 1] == 0u && ctl->remaining > 0u) ? 1 : 0;
  if (ctl->remaining == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = step + 1;
}

} // namespace sh
