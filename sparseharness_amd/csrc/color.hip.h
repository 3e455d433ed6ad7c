// color.hip.h -- kernels of sh_color: a greedy (first-fit) vertex colouring in a fixed priority order, by the work-efficient
// form of Jones-Plassmann (Jones, Plassmann, "A parallel graph coloring heuristic", SIAM J. Sci. Comput. 1993; the form
// with one counter per vertex and the orders R and LF: Hasenplaugh, Kaler, Schardl, Leiserson, "Ordering heuristics for
// parallel graph coloring", SPAA 2014).  color[v] is the smallest colour >= 0 that no neighbour PRECEDING v holds, which
// is what a serial loop over the vertices in that order gives (DESIGN.md "6l Greedy vertex colouring").
//
// The graph is sh_tri's simple undirected graph, kept as sh_core_graph's symmetric lists: ptr[rows + 1] / col[2M], every
// list strictly ascending, deg[v] = ptr[v + 1] - ptr[v].  THE ORDER is total: v precedes u when key(v) > key(u), key =
// (primary, tie) compared lexicographically (gcol_key: one 64-bit word).  primary(v) is prio[v] when the caller gives
// priorities, else deg[v] for order 2, else 0; tie(v) is "the smaller index first" for order 0 and "the larger
// mix32(v ^ seed) first" otherwise.  mix32 is a bijection of the 32-bit words, so no two vertices tie and every edge has
// exactly one end that precedes the other: the edges, directed from the preceding end, form a DAG.  A key is computed on
// the spot (one read of deg[u] or prio[u], none for orders 0 and 1 without prio); no key array is stored.
//
// The state of a call is wait[v], the number of neighbours preceding v that are not coloured yet, and color[v], -1 until
// v is COLOURED.  The launches:
//   gcol_init    color = -1, wait = 0; the vertices whose list is above GCOL_PIECE entries go to the far end of work
//                list 1 (empty until round 0 fills it) for gcol_count's piece class.
//   gcol_count   ONE pass over all lists: wait[v] = the number of entries u of v's list with key(u) > key(v).  Lists up to
//                GCOL_SHORT entries one lane, up to GCOL_PIECE one wave (both store their count), longer ones in pieces
//                of GCOL_PIECE, one wave per piece of a workgroup that takes the list whole, each piece adding its count
//                with one atomic.
//   gcol_ready   behind that kernel boundary: every v with wait[v] == 0 joins work list 0, the list of round 0.
//   gcol_assign  once per round, over the current list: ONE walk of v's list.  An entry u with color[u] >= 0 precedes v
//                (or it could not be coloured before v): its colour is marked as taken.  An entry u with color[u] < 0 is
//                preceded by v (or v would still wait for it): wait[u] gets ONE atomic decrement, and the one lane that
//                reads the old value 1 OWNS u and appends it to the next list.  Then color[v] = the smallest colour not
//                marked.  No key is compared in a round and NO RESTORE IS NEEDED: wait[u] counts exactly the preceding
//                neighbours of u, each of them is coloured in exactly one round and decrements exactly once, so the
//                word walks from its count down to 0 and never below, and exactly one decrement reads 1.
//   gcol_close   one workgroup: sums the WlParts, adds the round's vertices to `coloured`, folds the largest colour into
//                `colors`, empties the list just walked, swaps the lists, records the round and finishes when
//                coloured == rows.
//
// The smallest free colour is a reduction over the walk, which wl_expand cannot carry (its edge function returns
// nothing to the vertex): gcol_walk is a sibling traversal kept here, as truss_walk is kept in truss.hip.h.  Its classes:
//   a lane   (list <= GCOL_SHORT = 8 entries): the colour is at most 8, so a 32-bit mask in a register holds the marks.
//   a wave   (list <= GCOL_PIECE = 2048): the colour is at most 2048, so a bitmap of 2049 bits in LDS per wave does.
//   a workgroup (longer lists; they sit at the far end of the work list, filled downwards, as sh_truss's long items do,
//            so no list of pieces is stored): an LDS bitmap of `window` colours (the caller's; 0 means GCOL_WINDOW = 32768
//            bits, 4 KB).  When every colour of the window is taken the workgroup walks the list again for the next
//            window; ONLY THE FIRST WALK DECREMENTS.  The colour is at most the list's length, so this is bounded by
//            len / window + 1 walks.  The colours do not depend on the window.
//
// Invariant 1: EVERY VERTEX IS COLOURED ONCE AND JOINS A LIST ONCE.  A vertex joins list 0 in gcol_ready, by the one lane
// that looks at it, when nothing precedes it -- then nobody ever decrements its word, so it is never owned -- or it is
// appended by its owner, which is unique (above).  It is coloured by the visit of its list entry, in the round after.
// So the short entries of a list (from the front) and the long ones (from the far end) are at most `rows` together:
// A LIST OF `rows` PLACES CANNOT OVERFLOW, and `coloured` reaches `rows` exactly when every vertex has a colour.  Round
// r's list is exactly the vertices whose longest chain of preceding neighbours has r + 1 vertices: the rounds, the sizes
// and the edges per round depend on the graph and the order alone.
// TWO VERTICES OF ONE LIST ARE NEVER ADJACENT: of two neighbours one precedes the other, and the later one's word is
// above zero until the launch that colours the earlier one -- it joins the NEXT list at the earliest.  So no color[u]
// read in a launch is written in it: a walk reads the colours of earlier rounds (final) or -1, never a colour in the making.
// Invariant 2: NO KERNEL EVER WAITS for another kernel's write, and no lane for another lane's.  There is no spin loop,
// no retry and no compare-and-swap: a decrement is one atomic.  The gate words a launch reads (step, p, the current
// list's lengths) were written by a launch that ended before it; what a launch writes to the control block (the NEXT
// list's lengths) no workgroup of that same launch reads as a gate.  Values are written with vector stores, atomics or
// plain C++ only.  max_rounds bounds the call.
// Invariant 3: EVERY LOOP IS BOUNDED.  The strided loops by the list length or `rows`; a list walk by the list's length;
// the windows of a long list by len / window + 1; the search of a bitmap by its words.
//
// Worst cases.  The number of rounds is the longest chain in the order, not the diameter: the natural order on a path
// takes n rounds, each of which costs its launches however small its list is; K_n takes n rounds under every order, with
// n walks of n - 1 entries, and its last vertex's word is hit by n - 1 decrements.  A long list whose colour lies beyond
// the first window is walked once per window up to its colour.  A hub's word takes one atomic per preceding neighbour.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int GCOL_SHORT = 8;             // lists up to this many entries: one lane each, the marks in a register
constexpr int GCOL_PIECE = 2048;          // lists up to this: one wave, the marks in LDS; above: a workgroup, in windows
constexpr int GCOL_BATCH = 32;            // rounds enqueued ahead of the host at most (the first batch holds 8)
constexpr int GCOL_MAX_BLOCKS = 1024;     // workgroups of a launch at most: one WlPart each
constexpr int GCOL_CTL_BYTES = 1024;      // device bytes set aside for ColorCtl
constexpr int GCOL_PART_BYTES = 16 * GCOL_MAX_BLOCKS;
constexpr int GCOL_WINDOW = 32768;        // colours per window of a workgroup's bitmap at most, and the default (4 KB of LDS)
constexpr int GCOL_WAVE_WORDS = GCOL_PIECE / 32 + 1;   // a wave's bitmap: colours 0 .. GCOL_PIECE

struct ColorRec {   // what round k of a batch did (read back by the host once per batch)
  int32_t ran;
  uint32_t size, edges, pad;
};
// Control block in device memory.
struct ColorCtl {
  uint32_t n[2], nl[2];          // work list 0 / 1: its short entries (from the front), its long ones (from the far end)
  uint32_t nsl;                  // the long lists of gcol_count (at the far end of list 1, which is empty then)
  int32_t p;                     // the list the next round walks (the other one is filled meanwhile)
  int32_t step;                  // the round that runs next (-1 once the run has finished)
  int32_t finished;
  uint32_t coloured;             // vertices that have a colour
  int32_t colors;                // the largest colour given so far, plus 1
  ColorRec rec[GCOL_BATCH];
};
// The WlPart of a workgroup of gcol_assign: a = list entries looked at (the sum of the list lengths of its vertices),
// b = the largest colour it gave, plus 1 (0: it gave none).

struct ColorGraph {   // the handle's lists, as a kernel argument
  int32_t rows;
  const int32_t *ptr, *col;
};
struct ColorLists { uint32_t *list[2]; };   // `rows` places each
// The order of a call.  prim: the caller's prio, or deg for order 2, or NULL (every primary 0).
struct ColorOrder {
  const int32_t *prim;
  int32_t order;
  uint32_t seed;
};

// A bijection of the 32-bit words (every step is one: an xor with a shifted copy, a multiplication by an odd number).
__host__ __device__ __forceinline__ uint32_t gcol_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// v precedes u exactly when gcol_key(v) > gcol_key(u): the primary (signed, so its sign bit is flipped) above the tie.
__device__ __forceinline__ uint64_t gcol_key(const ColorOrder &O, int32_t v) {
  const uint32_t hi = (uint32_t)(O.prim ? O.prim[v] : 0) ^ 0x80000000u;
  const uint32_t lo = O.order == 0 ? ~(uint32_t)v : gcol_mix32((uint32_t)v ^ O.seed);
  return ((uint64_t)hi << 32) | lo;
}
// v joins a work list: at the front, or at the far end when its list is of the workgroup class.  (Any control flow.)
__device__ __forceinline__ void gcol_push(ColorCtl *ctl, int q, uint32_t *__restrict__ list, int32_t rows, int32_t v, int32_t len) {
  if (len > GCOL_PIECE) list[(int64_t)rows - 1 - (int64_t)wl_append_here(&ctl->nl[q])] = (uint32_t)v;
  else list[wl_append_here(&ctl->n[q])] = (uint32_t)v;
}

// color = -1 and wait = 0 for every row; the long lists of gcol_count.  (The host has zeroed the control block: step = 0,
// p = 0, both lists empty, nothing coloured, no colour given.)
__global__ __launch_bounds__(WL_BS) void gcol_init(ColorCtl *ctl, ColorGraph G, int32_t *__restrict__ wait, int32_t *__restrict__ color,
                                                    uint32_t *__restrict__ far) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool on = v < G.rows;
    if (on) { color[v] = -1; wait[v] = 0; }
    const bool heavy = on && G.ptr[v + 1] - G.ptr[v] > GCOL_PIECE;
    const uint32_t at = wl_wave_append(&ctl->nsl, heavy, lane);
    if (heavy) far[-(int64_t)at] = (uint32_t)v;
  }
}

// wait[v] = the neighbours that precede v.
__global__ __launch_bounds__(WL_BS) void gcol_count(const ColorCtl *ctl, ColorGraph G, ColorOrder O, int32_t *wait,
                                                     const uint32_t *__restrict__ far) {
  const int lane = wl_lane();
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool on = v < G.rows;
    const int32_t s = on ? G.ptr[v] : 0;
    int32_t len = on ? G.ptr[v + 1] - s : 0;
    if (len > GCOL_PIECE) len = 0;   // (left to the long lists below)
    const uint64_t kv = on ? gcol_key(O, (int32_t)v) : 0ull;
    if (on && len <= GCOL_SHORT) {
      int32_t cnt = 0;
      for (int32_t j = 0; j < len; j++) cnt += gcol_key(O, G.col[s + j]) > kv ? 1 : 0;
      if (len > 0) wait[v] = cnt;
    }
    uint64_t m = __ballot(len > GCOL_SHORT);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sb = __shfl(s, src), lb = __shfl(len, src);
      const uint64_t kb = (uint64_t)__shfl((unsigned long long)kv, src);
      uint32_t cnt = 0;
      for (int32_t j = lane; j < lb; j += 64) cnt += gcol_key(O, G.col[sb + j]) > kb ? 1u : 0u;
      cnt = wl_wave_sum(cnt);
      if (lane == src) wait[v] = (int32_t)cnt;
    }
  }
  const int64_t nsl = (int64_t)ctl->nsl;
  for (int64_t h = blockIdx.x; h < nsl; h += gridDim.x) {   // a long list: one workgroup, one wave per piece in turn
    const int32_t v = (int32_t)far[-h];
    const int32_t s = G.ptr[v], len = G.ptr[v + 1] - s;
    const uint64_t kv = gcol_key(O, v);
    for (int32_t off = (int32_t)(threadIdx.x >> 6) * GCOL_PIECE; off < len; off += (WL_BS / 64) * GCOL_PIECE) {
      const int32_t end = min(off + GCOL_PIECE, len);
      uint32_t cnt = 0;
      for (int32_t j = off + lane; j < end; j += 64) cnt += gcol_key(O, G.col[s + j]) > kv ? 1u : 0u;
      cnt = wl_wave_sum(cnt);
      if (lane == 0 && cnt) (void)__hip_atomic_fetch_add(&wait[v], (int32_t)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The list of round 0: every vertex that nothing precedes (list 0; gcol_count has ended, so list 1's far end is free again).
__global__ __launch_bounds__(WL_BS) void gcol_ready(ColorCtl *ctl, ColorGraph G, const int32_t *__restrict__ wait, ColorLists L) {
  const int lane = wl_lane();
  uint32_t *__restrict__ list = L.list[0];
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t v = base + lane;
    const bool take = v < G.rows && wait[v] == 0;
    const int32_t len = take ? G.ptr[v + 1] - G.ptr[v] : 0;
    const uint32_t at = wl_wave_append(&ctl->n[0], take && len <= GCOL_PIECE, lane);
    const uint32_t atl = wl_wave_append(&ctl->nl[0], take && len > GCOL_PIECE, lane);
    if (take) {   // (only this lane looks at v, and v is in no list: invariant 1)
      if (len > GCOL_PIECE) list[(int64_t)G.rows - 1 - (int64_t)atl] = (uint32_t)v;
      else list[at] = (uint32_t)v;
    }
  }
}

// The walk of a round: the short entries list[0, n), then the long ones list[rows - 1], list[rows - 2], ... (nl of them),
// one workgroup each.  taken(u) >= 0: the colour of a coloured neighbour; otherwise it has done what an uncoloured one
// gets (`first`: on the first walk of the list only) and returns -1.  give(v, c) stores v's colour.  -> the lane's sum of
// list lengths.  `window`: a multiple of 64 in [64, GCOL_WINDOW].
template <class Taken, class Give>
__device__ __forceinline__ uint32_t gcol_walk(const ColorGraph &G, const uint32_t *__restrict__ list, int64_t n, int64_t nl, int32_t window,
                                              Taken taken, Give give) {
  __shared__ uint32_t s_wave[WL_BS / 64][GCOL_WAVE_WORDS];
  __shared__ uint32_t s_win[GCOL_WINDOW / 32];
  const int lane = wl_lane(), wv = (int)(threadIdx.x >> 6);
  uint32_t looked = 0;
  for (int64_t base = wl_wave() * 64; base < n; base += wl_waves() * 64) {
    const bool valid = base + lane < n;
    const int32_t v = valid ? (int32_t)list[base + lane] : 0;
    const int32_t s = valid ? G.ptr[v] : 0;
    const int32_t len = valid ? G.ptr[v + 1] - s : 0;   // (<= GCOL_PIECE: gcol_push)
    looked += (uint32_t)len;
    if (valid && len <= GCOL_SHORT) {
      uint32_t mask = 0;
      for (int32_t j = 0; j < len; j++) {
        const int32_t c = taken(G.col[s + j], true);
        if (c >= 0 && c < 32) mask |= 1u << c;
      }
      give(v, __ffs((int)~mask) - 1);   // (at most 8 marks: a bit of the low nine is free)
    }
    uint64_t m = __ballot(len > GCOL_SHORT);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t vb = __shfl(v, src), sb = __shfl(s, src), lb = __shfl(len, src);
      const int words = lb / 32 + 1;   // colours 0 .. lb
      uint32_t *bm = s_wave[wv];
      for (int w = lane; w < words; w += 64) bm[w] = 0u;
      wl_wave_sync();
      for (int32_t j = lane; j < lb; j += 64) {
        const int32_t c = taken(G.col[sb + j], true);
        if (c >= 0 && c <= lb) (void)__hip_atomic_fetch_or(&bm[c >> 5], 1u << (c & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      wl_wave_sync();
      uint32_t best = 0xFFFFFFFFu;
      for (int w = lane; w < words; w += 64) {
        const uint32_t free_bits = ~bm[w];
        if (free_bits) best = min(best, (uint32_t)(w * 32 + __ffs((int)free_bits) - 1));
      }
      best = wl_wave_min(best);   // (lb entries mark at most lb of the lb + 1 colours the words hold)
      if (lane == 0) give(vb, (int32_t)best);
      wl_wave_sync();           // (the bitmap is read before the next list clears it)
    }
  }
  for (int64_t h = blockIdx.x; h < nl; h += gridDim.x) {   // a long list: the whole workgroup, a window of colours per walk
    const int32_t v = (int32_t)list[(int64_t)G.rows - 1 - h];
    const int32_t s = G.ptr[v], len = G.ptr[v + 1] - s;
    if (threadIdx.x == 0) looked += (uint32_t)len;
    for (int32_t lo = 0; lo <= len; lo += window) {   // at most len / window + 1 walks: the colour is at most len
      for (int w = (int)threadIdx.x; w < window / 32; w += WL_BS) s_win[w] = 0u;
      __syncthreads();
      for (int32_t j = (int32_t)threadIdx.x; j < len; j += WL_BS) {
        const int32_t c = taken(G.col[s + j], lo == 0);
        if (c >= lo && c - lo < window)
          (void)__hip_atomic_fetch_or(&s_win[(c - lo) >> 5], 1u << ((c - lo) & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();
      uint32_t best = 0xFFFFFFFFu;
      for (int w = (int)threadIdx.x; w < window / 32; w += WL_BS) {
        const uint32_t free_bits = ~s_win[w];
        if (free_bits) best = min(best, (uint32_t)(w * 32 + __ffs((int)free_bits) - 1));
      }
      best = wl_block_fold<WlMin>(best);
      __syncthreads();   // (the bitmap is read before the next walk or list writes it)
      if (best != 0xFFFFFFFFu) {   // (the same word in every thread)
        if (threadIdx.x == 0) give(v, lo + (int32_t)best);
        break;
      }
    }
  }
  return looked;
}

// Round s: colours the work list's vertices and takes one from the word of every neighbour they precede.
__global__ __launch_bounds__(WL_BS) void gcol_assign(ColorCtl *ctl, int s, ColorGraph G, int32_t window, int32_t *wait, int32_t *color,
                                                      ColorLists L, WlPart *__restrict__ part) {
  if (ctl->step != s) return;
  const int p = ctl->p, q = p ^ 1;
  uint32_t *__restrict__ next = L.list[q];
  uint32_t most = 0;   // the largest colour this lane gave, plus 1
  const uint32_t looked = gcol_walk(G, L.list[p], (int64_t)ctl->n[p], (int64_t)ctl->nl[p], window,
      [&](int32_t u, bool first) {
        const int32_t c = wl_load(&color[u]);   // (not written in this launch: u is in another round's list)
        if (c < 0 && first && __hip_atomic_fetch_add(&wait[u], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1)
          gcol_push(ctl, q, next, G.rows, u, G.ptr[u + 1] - G.ptr[u]);   // this lane owns u
        return c;
      },
      [&](int32_t v, int32_t c) {
        color[v] = c;
        most = max(most, (uint32_t)c + 1u);
      });
  wl_block_part<WlMax>(part, looked, most);
}

// Closes round s (slot r of the batch).  One workgroup folds the WlParts (no atomics on one word) and its first lane
// records the round and decides.
__global__ __launch_bounds__(WL_BS) void gcol_close(ColorCtl *ctl, int r, int s, int32_t rows, int nparts, const WlPart *__restrict__ part) {
  if (!wl_from_thread0(ctl->step == s)) return;
  const WlPart sums = wl_sum_parts<WlMax>(part, nparts);
  if (threadIdx.x != 0) return;
  const uint32_t looked = sums.a, most = sums.b;
  const int p = ctl->p;
  const uint32_t size = ctl->n[p] + ctl->nl[p];
  ctl->rec[r] = ColorRec{1, size, looked, 0u};
  ctl->coloured += size;
  ctl->colors = max(ctl->colors, (int32_t)most);
  ctl->n[p] = 0u; ctl->nl[p] = 0u;
  ctl->p = p ^ 1;
  if (ctl->coloured == (uint32_t)rows) { ctl->finished = 1; ctl->step = -1; return; }
  ctl->step = s + 1;
}

} // namespace sh
