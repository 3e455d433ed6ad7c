// match.hip.h -- kernels of sh_match: the greedy weighted matching of the simple undirected graph under a square matrix,
// the values as weights, in rounds of locally dominant edges on a flat list of edges (Preis, "Linear time
// 1/2-approximation algorithm for maximum weighted matching in general graphs", STACS 1999; Hoepman, "Simple distributed
// weighted matchings", 2004; Manne and Bisseling, "A parallel approximation algorithm for the weighted maximum matching
// problem", PPAM 2007).  mate[v] becomes the partner of v or -1, in_match[e] 1 for the matched edges (DESIGN.md "6n
// Greedy matching").
//
// The graph, the edges eu / ev, k(b) and wk[e] = k(weight[e]) are sh_msf's (msf.hip.h; the handle is built by the same
// code).  Two scalars of the call fix the order: MKEY(e) = hi(e) << 32 | lo(e) with hi = wk[e] for heavy == 0 (lightest
// first) and ~wk[e] for heavy == 1 (heaviest first), lo = e for seed == 0 and mix32(e ^ seed) otherwise (sh_color's
// gcol_mix32).  Both forms of lo are bijections of e, so NO TWO KEYS ARE EQUAL and the answer is unique: THE MATCHING
// THAT A SERIAL LOOP RETURNS WHEN IT TAKES THE EDGES IN ASCENDING MKEY AND KEEPS AN EDGE WHEN BOTH ITS ENDS ARE STILL
// FREE.  Every result is compared with ==.
//     A key may be all ones, MATCH_MAX.  For seed == 0 it cannot (e < 2^31).  For seed != 0, e = unmix32(~0) ^ seed may
//     be an edge, and if its weight is the last of the order (the bits 0x7FFFFFFF for heavy == 0, 0xFFFFFFFF for heavy
//     == 1) its key is MATCH_MAX.  That is harmless and nothing is masked: no key is ABOVE MATCH_MAX, a bid of MATCH_MAX
//     leaves the word as it is, and match_take never asks "was there a bid" but "is best == my key" of an edge it holds.
//     best[u] == MATCH_MAX == MKEY(e) at both ends says that no other kept edge at u or v bid below e, and all others
//     are below: e is the one kept edge there, and dominant.
//
// State: mate[rows] (the caller's vector), best[v] one 64-bit word per vertex, eu[M] / ev[M] / wk[M], two work lists of M
// edge ids.  The work item is an edge of a flat list: no long rows, no pieces, one lane per edge.  A ROUND is one step of
// the control block, four launches, each of which returns at once unless the control block gives it work:
//   match_bid    best[v] == MATCH_MAX FOR EVERY FREE VERTEX WITH A LISTED EDGE was written by a launch that ended before
//                this one.  For every edge e of the list: if mate[eu[e]] or mate[ev[e]] is set the edge is dropped for
//                good.  Otherwise it is KEPT: appended to the next list with a wave-aggregated push, and MKEY(e) goes
//                into best[eu[e]] and best[ev[e]] with the pre-checked 64-bit atomic minimum (msf_lower).  Reads mate,
//                writes best.
//   match_take   walks the NEXT list.  Edge e is matched when best[eu[e]] == MKEY(e) && best[ev[e]] == MKEY(e): it is
//                the smallest kept key at both its ends (locally dominant).  THE EDGE TESTS ITSELF, so nothing has to
//                invert mix32.  It stores mate[eu] = ev, mate[ev] = eu, in_match[e] = 1; two matched edges share no end
//                (both would be best there, and keys differ), so no two lanes store to one word.  Reads best, writes
//                mate: NEITHER LAUNCH READS WHAT IT WRITES ITSELF, and they alternate.
//   match_clear  best = MATCH_MAX for both ends of every edge of the next list (lanes that meet on a word store the same
//                value).  The edges of the NEXT round's next list are a subset of these, so the bid's precondition
//                holds.  A vertex whose edges were all dropped keeps no stale word either -- its last kept edge cleared
//                it -- and were one left, nobody would read it: only ends of kept edges are bid for or tested.
//   match_close  one workgroup sums the workgroups' counts, records the round as walked (the list's length), kept,
//                matched, and swaps the lists.  THE RUN FINISHES AT THE FIRST ROUND THAT KEPT NO EDGE (take and clear
//                return at once in that round).
// match_init sets mate = -1, best = MATCH_MAX, list 0 = all edges, in_match = 0 and the optional weight.
//
// Why that is right, by induction over the rounds: every edge matched so far is in the greedy matching, and every edge
// dropped so far is not.  Let (u, v) be dominant in round r.  Both ends are free (it was kept).  Suppose greedy did not
// take it: then greedy took, earlier, an edge (u, w) -- or one at v -- with a smaller key.  (u, w) is not kept in round r
// (it would have bid below (u, v) at u), so it was dropped before: w was matched through some (w, x) while u was free.
// By induction (w, x) is in the greedy matching, so greedy cannot take (u, w) as well: a contradiction.  (Said forwards:
// an edge (u, w) that died at u before (u, v) became dominant died because w was matched through (w, x), which was
// dominant while (u, w) was still kept, so its key is smaller; greedy reached (w, x) first and took it, never takes
// (u, w), and finds u and v free when it reaches (u, v).)  A dropped edge has a matched end, and matched edges are
// greedy's, so greedy does not take it.  The run ends when no edge has two free ends: the matching is maximal, and it is
// greedy's.
//
// bid sees one state of mate, so the kept edges, best, the matched edges, the rounds, walked, kept and matched of every
// round, mate and in_match are functions of the input, heavy and seed alone; only the order inside a list and the times
// may differ from run to run.  Every round that keeps an edge matches one (the smallest kept key of all is dominant) and
// a pair uses two vertices: rounds <= floor(rows / 2) + 1, the empty last one included, attained by a path whose keys
// ascend along it.  Equal weights with seed == 0 make such paths everywhere (one pair per round in places): that is
// what seed is for.
//
// Invariant 1: NO LIST CAN OVERFLOW ON ANY INPUT.  An edge enters a list once per round, by the one lane that holds it:
// M places suffice.
// Invariant 2: NO KERNEL EVER WAITS FOR ANOTHER KERNEL'S WRITE, and no lane for another lane's.  There is no
// compare-and-swap, no retry and no spin loop; the words a launch reads were written by a launch that ended before it,
// and no kernel reads a word that another lane of the same launch writes, unless every writer stores the same value
// (best under the atomic minimum is only compared with a key that can no longer rise).  Values are written with vector
// stores or plain C++ only.
#pragma once
#include "color.hip.h"   // gcol_mix32
#include "msf.hip.h"     // MsfEdges, MsfLists, msf_unkey, msf_lower

namespace sh {

constexpr int MATCH_BATCH = 32;          // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int MATCH_MAX_BLOCKS = 1024;   // workgroups of a launch at most: one WlPart each
constexpr int MATCH_CTL_BYTES = 1024;    // device bytes set aside for MatchCtl
constexpr int MATCH_PART_BYTES = 16 * MATCH_MAX_BLOCKS;
constexpr uint64_t MATCH_MAX = 0xFFFFFFFFFFFFFFFFull;   // no bid (or the bid of the one key that is all ones, see above)

struct MatchRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran;
  uint32_t walked, kept, matched;
};
// Control block in device memory.
struct MatchCtl {
  uint32_t n[2];                 // the lengths of work list 0 / 1
  int32_t p;                     // the list the next round walks (the other one is filled meanwhile)
  int32_t step;                  // the round that runs next (-1 once the run has finished)
  int32_t finished;
  uint32_t pad[3];
  MatchRec rec[MATCH_BATCH];
};
// The WlPart of a workgroup.  match_take: a = edges matched.

struct MatchOrder { uint32_t flip, seed; };   // flip: 0 (heavy == 0) or 0xFFFFFFFF (heavy == 1)

__device__ __forceinline__ uint64_t match_key(const MsfEdges &E, const MatchOrder &O, uint32_t e) {
  const uint32_t hi = E.wk[e] ^ O.flip;
  const uint32_t lo = O.seed == 0u ? e : gcol_mix32(e ^ O.seed);
  return ((uint64_t)hi << 32) | (uint64_t)lo;
}

// Every vertex free, no bid anywhere, list 0 = all edges, no edge matched; weight[e] (if wanted) = the bits of the entry
// that gave wk[e].  (The host has zeroed the control block: step = 0, p = 0.)
__global__ __launch_bounds__(WL_BS) void match_init(MatchCtl *ctl, int32_t rows, MsfEdges E, int32_t *__restrict__ mate,
                                                    uint64_t *__restrict__ best, uint32_t *__restrict__ list0,
                                                    int32_t *__restrict__ in_match, uint32_t *__restrict__ weight) {
  const int64_t n = max(rows, E.M);
  for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WL_BS) {
    if (i < rows) { mate[i] = -1; best[i] = MATCH_MAX; }
    if (i < E.M) {
      list0[i] = (uint32_t)i;
      if (in_match) in_match[i] = 0;
      if (weight) weight[i] = msf_unkey(E.wk[i]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n[0] = (uint32_t)E.M;
}

// Round s: the edges of the list whose ends are both free go on to the next list and bid for both ends.
__global__ __launch_bounds__(WL_BS) void match_bid(MatchCtl *ctl, int s, MsfEdges E, MatchOrder O, const int32_t *__restrict__ mate,
                                                   uint64_t *best, MsfLists L) {
  if (ctl->step != s) return;
  const int pl = ctl->p, q = pl ^ 1;
  const int64_t n = ctl->n[pl];
  const uint32_t *__restrict__ list = L.list[pl];
  uint32_t *__restrict__ next = L.list[q];
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const uint32_t e = valid ? list[base + lane] : 0u;
    const int32_t u = valid ? E.eu[e] : 0, v = valid ? E.ev[e] : 0;
    const bool keep = valid && mate[u] < 0 && mate[v] < 0;
    const uint32_t at = wl_wave_append(&ctl->n[q], keep, lane);
    if (keep) {   // (only this lane holds e in this round: invariant 1)
      next[at] = e;
      const uint64_t key = match_key(E, O, e);
      msf_lower(&best[u], key);
      msf_lower(&best[v], key);
    }
  }
}

// Round s: every kept edge that holds both its ends' words is matched.  Reads best, writes mate and in_match.
__global__ __launch_bounds__(WL_BS) void match_take(const MatchCtl *ctl, int s, MsfEdges E, MatchOrder O,
                                                    const uint64_t *__restrict__ best, int32_t *__restrict__ mate,
                                                    int32_t *__restrict__ in_match, MsfLists L, WlPart *__restrict__ part) {
  if (ctl->step != s) return;
  const int q = ctl->p ^ 1;
  const int64_t n = ctl->n[q];
  if (n == 0) return;
  const uint32_t *__restrict__ next = L.list[q];
  uint32_t matched = 0;
  for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WL_BS) {
    const uint32_t e = next[i];
    const int32_t u = E.eu[e], v = E.ev[e];
    const uint64_t key = match_key(E, O, e);
    if (best[u] == key && best[v] == key) {
      mate[u] = v;
      mate[v] = u;
      if (in_match) in_match[e] = 1;
      matched++;
    }
  }
  wl_block_part(part, matched, 0u);
}

// Round s: no bid is left at the ends of the kept edges (the only words of best that hold one).
__global__ __launch_bounds__(WL_BS) void match_clear(const MatchCtl *ctl, int s, MsfEdges E, uint64_t *__restrict__ best, MsfLists L) {
  if (ctl->step != s) return;
  const int q = ctl->p ^ 1;
  const int64_t n = ctl->n[q];
  const uint32_t *__restrict__ next = L.list[q];
  for (int64_t i = (int64_t)blockIdx.x * WL_BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WL_BS) {
    const uint32_t e = next[i];
    best[E.eu[e]] = MATCH_MAX;   // (whoever stores here stores the same word)
    best[E.ev[e]] = MATCH_MAX;
  }
}

// Closes round s (slot k of the batch).  One workgroup sums the WlParts (no atomics on one word) and its first lane
// records the round, swaps the lists and decides.
__global__ __launch_bounds__(WL_BS) void match_close(MatchCtl *ctl, int k, int s, int nparts, const WlPart *__restrict__ part) {
  if (!wl_from_thread0(ctl->step == s)) return;
  const int pl = ctl->p, q = pl ^ 1;
  const uint32_t kept = ctl->n[q];
  const uint32_t matched = wl_sum_parts(part, kept ? nparts : 0).a;   // (the parts are this round's only if take ran)
  if (threadIdx.x != 0) return;
  ctl->rec[k] = MatchRec{1, ctl->n[pl], kept, matched};
  ctl->n[pl] = 0u;
  ctl->p = q;
  if (kept == 0u) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = s + 1;
}

} // namespace sh
