// tri.hip.h -- kernels of sh_tri: exact triangle counts per vertex and in total, by intersecting forward lists (the
// forward algorithm: Schank, Wagner, "Finding, counting and listing all triangles in large graphs", WEA 2005; the degree
// orientation and its sqrt(2M) bound: Chiba, Nishizeki, "Arboricity and subgraph listing algorithms", SIAM J. Comput.
// 1985; Latapy, "Main-memory triangle computations for very large (sparse (power-law)) graphs", TCS 2008).  In semiring
// words the total is the sum of (L . L) o L on (+,x), L the oriented pattern: the mask makes the product an
// intersection (DESIGN.md "6i Triangle counting").
//
// The graph lives as fwd_ptr[rows + 1] / fwd_col[M]: N+(v), the forward list of v, holds the neighbours of v that
// come after v in the orientation's order (a strict total order on the vertices), STRICTLY ASCENDING by index.  The
// handle is built by worklist.hip.h's kernels (wl_und_flag<BfsKeep>, ... wl_forward_lists).
//
// Invariant 1: EVERY TRIANGLE IS FOUND ONCE.
//   A triangle's three vertices are a < b < c in the orientation's order, in exactly one way (the order is total).
//   Its edges are then stored as b in N+(a), c in N+(a), c in N+(b), and in no other forward list.
//   The count looks, for every forward edge x -> y, at the elements z of N+(x) and N+(y): z needs x < y < z, so
//   (x, y, z) = (a, b, c), at the edge a -> b alone, and c stands in either list once (no parallel edges).
// Invariant 2: NO KERNEL EVER WAITS for another kernel's write, nor a lane for another lane's; EVERY LOOP IS BOUNDED
// BY A LIST LENGTH (or by its logarithm: the bisections).  Sums meet in 64-bit integer adds, which are associative:
// nothing depends on who adds first.  Values are written with vector stores, ordinary atomics or plain C++ only.
//
// The work item is a source vertex a with its whole forward list; its class is its list's length n:
//   n <= TRI_SHORT              one lane: for every b of N+(a), every other c of N+(a) is bisected into N+(b) in memory.
//   TRI_SHORT < n <= TRI_WAVE   one wave: N+(a) is staged in LDS once; for every b the wave streams N+(b) with coalesced
//                               loads and every lane bisects its entry into the staged list.
//   n > TRI_WAVE                one workgroup (tri_count_heavy): N+(a) is staged in chunks of at most TRI_CHUNK entries;
//                               per chunk the workgroup's waves take the b of the WHOLE list in turn, stream N+(b) and
//                               bisect into the chunk.  ANY LENGTH goes this way: there is no other path for a list
//                               that is longer still.
// Accumulation: one 64-bit add to tri[c] per hit; the hits of edge a -> b (of one chunk, in the heavy class) are counted
// across the wave by ballot and added once to tri[b]; those of all of a's edges once to tri[a] (per wave of the
// workgroup in the heavy class).  The total and `probes` go into one TriPart per workgroup; tri_finish adds them up
// (no adds to one word from thousands of waves: they retire about 6 ns apart, see frontier_detect).
// With PER_VERTEX = false (tri == NULL) the adds to tri are not compiled in.
//
// probes counts list entries looked at, each time one is looked at: the entries of N+(a) once (as they are staged, or
// as the lane walks them), every streamed entry of an N+(b) once, and every entry a bisection compares with.
#pragma once
#include "worklist.hip.h"

namespace sh {

constexpr int TRI_SHORT = 8;             // forward lists up to this many entries: one lane each
constexpr int TRI_WAVE = 512;            // up to this many: one wave each, the list staged in LDS (2 KB per wave)
constexpr int TRI_CHUNK = 2048;          // the workgroup class stages this many entries at a time (8 KB)
constexpr int TRI_DEAL = 16;             // tri_count_heavy deals the rows to the workgroups in runs of this many
constexpr int TRI_MAX_BLOCKS = 1024;     // workgroups of a launch at most: one TriPart each
constexpr int TRI_CTL_BYTES = 256;       // device bytes set aside for TriCtl
constexpr int TRI_PART_BYTES = 16 * TRI_MAX_BLOCKS;   // per counting kernel

struct TriPart { uint64_t hits, probes; };   // a workgroup's sums
struct TriCtl {                              // control block in device memory
  uint64_t triangles, probes;
  uint32_t max_forward;                      // written once, by the build
};

struct TriGraph {   // the handle's lists, as a kernel argument
  int32_t rows;
  const int32_t *fwd_ptr, *fwd_col;
};

__device__ __forceinline__ void tri_add(uint64_t *tri, int32_t v, uint64_t n) {
  (void)__hip_atomic_fetch_add(&tri[v], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Is c among the n ascending entries of s (LDS or memory)?  At most 32 steps; *looked += the entries compared with.
template <class P>
__device__ __forceinline__ bool tri_find(P s, uint32_t n, int32_t c, uint32_t *looked) {
  uint32_t lo = 0, seen = 0;   // lo = how many entries are known to be smaller than c
  for (uint32_t step = n ? 1u << (31 - __clz((int)n)) : 0u; step; step >>= 1) {
    const uint32_t m = lo + step;
    if (m <= n) {
      seen++;
      if (s[m - 1] < c) lo = m;
    }
  }
  bool hit = false;
  if (lo < n) { seen++; hit = s[lo] == c; }
  *looked += seen;
  return hit;
}

// The wave streams N+(b) = col[sb, sb + lb) and bisects every entry into the n staged entries of s -> the hits, the
// same number in every lane.
template <bool PER_VERTEX>
__device__ __forceinline__ uint32_t tri_stream(const int32_t *__restrict__ col, int32_t sb, int32_t lb, const int32_t *s, uint32_t n,
                                               uint64_t *tri, uint32_t *looked) {
  const int lane = wl_lane();
  uint32_t hits = 0;
  for (int32_t j0 = 0; j0 < lb; j0 += 64) {   // (wave-uniform bounds: the ballot sees every lane)
    const int32_t j = j0 + lane;
    bool hit = false;
    if (j < lb) {
      const int32_t c = col[sb + j];
      *looked += 1u;
      hit = tri_find(s, n, c, looked);
      if (PER_VERTEX && hit) tri_add(tri, c, 1ull);
    }
    hits += (uint32_t)__popcll(__ballot(hit));
  }
  return hits;
}

// The lane and the wave classes, over all rows: a wave takes 64 rows at a time.
template <bool PER_VERTEX>
__global__ __launch_bounds__(WL_BS) void tri_count_light(TriGraph G, uint64_t *tri, TriPart *__restrict__ part) {
  __shared__ int32_t s_list[WL_BS / 64][TRI_WAVE];
  int32_t *mine = s_list[threadIdx.x >> 6];
  const int32_t *__restrict__ ptr = G.fwd_ptr, *__restrict__ col = G.fwd_col;
  const int lane = wl_lane();
  uint64_t hits = 0, probes = 0;   // this lane's share (a wave's sums are kept by its lane 0)
  for (int64_t base = wl_wave() * 64; base < G.rows; base += wl_waves() * 64) {
    const int64_t a = base + lane;
    const int32_t s = a < G.rows ? ptr[a] : 0;
    const int32_t n = a < G.rows ? ptr[a + 1] - s : 0;
    if (n > 1 && n <= TRI_SHORT) {   // (a list of one entry closes no triangle)
      uint32_t ha = 0, looked = (uint32_t)n;
      for (int32_t i = 0; i < n; i++) {
        const int32_t b = col[s + i];
        const int32_t sb = ptr[b], lb = ptr[b + 1] - sb;
        if (lb == 0) continue;
        uint32_t hb = 0;
        for (int32_t k = 0; k < n; k++) {
          if (k == i) continue;
          const int32_t c = col[s + k];
          if (tri_find(col + sb, (uint32_t)lb, c, &looked)) {
            hb++;
            if (PER_VERTEX) tri_add(tri, c, 1ull);
          }
        }
        if (PER_VERTEX && hb) tri_add(tri, b, hb);
        ha += hb;
      }
      if (PER_VERTEX && ha) tri_add(tri, (int32_t)a, ha);
      hits += ha; probes += looked;
    }
    uint64_t m = __ballot(n > TRI_SHORT && n <= TRI_WAVE);
    while (m) {
      const int src = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int32_t sa = __shfl(s, src), na = __shfl(n, src);
      for (int32_t i = lane; i < na; i += 64) mine[i] = col[sa + i];
      wl_wave_sync();
      uint32_t looked = 0;
      uint64_t ha = 0;
      for (int32_t i = 0; i < na; i++) {
        const int32_t b = mine[i];
        const int32_t sb = ptr[b], lb = ptr[b + 1] - sb;
        const uint32_t hb = tri_stream<PER_VERTEX>(col, sb, lb, mine, (uint32_t)na, tri, &looked);
        if (PER_VERTEX && hb && lane == 0) tri_add(tri, b, hb);
        ha += hb;
      }
      wl_wave_sync();   // (before the next list overwrites the staged one)
      probes += looked;
      if (lane == 0) {
        if (PER_VERTEX && ha) tri_add(tri, (int32_t)(base + src), ha);
        hits += ha; probes += (uint64_t)na;
      }
    }
  }
  hits = wl_block_fold<WlSum>(hits);
  probes = wl_block_fold<WlSum>(probes);
  if (threadIdx.x == 0) part[blockIdx.x] = TriPart{hits, probes};
}

// The workgroup class.  The rows are dealt to the workgroups in runs of TRI_DEAL (neighbouring hubs go to different
// workgroups); a workgroup looks at WL_BS of its rows at a time, notes those of its class and takes them one by one.
template <bool PER_VERTEX>
__global__ __launch_bounds__(WL_BS) void tri_count_heavy(TriGraph G, uint64_t *tri, TriPart *__restrict__ part) {
  __shared__ int32_t s_chunk[TRI_CHUNK];
  __shared__ int32_t s_todo[WL_BS];
  __shared__ uint32_t s_ntodo;
  const int32_t *__restrict__ ptr = G.fwd_ptr, *__restrict__ col = G.fwd_col;
  const int lane = wl_lane(), wave = (int)(threadIdx.x >> 6);
  uint64_t hits = 0, probes = 0;
  const int64_t runs = ((int64_t)G.rows + TRI_DEAL - 1) / TRI_DEAL;   // runs of rows; this workgroup's: blockIdx.x + k * gridDim.x
  constexpr int RUNS_AT_ONCE = WL_BS / TRI_DEAL;
  for (int64_t k0 = 0; (k0 * (int64_t)gridDim.x + blockIdx.x) < runs; k0 += RUNS_AT_ONCE) {   // (workgroup-uniform)
    if (threadIdx.x == 0) s_ntodo = 0u;
    __syncthreads();
    const int64_t run = (k0 + (int64_t)(threadIdx.x / TRI_DEAL)) * gridDim.x + blockIdx.x;
    const int64_t r = run * TRI_DEAL + (int64_t)(threadIdx.x % TRI_DEAL);
    if (run < runs && r < G.rows && ptr[r + 1] - ptr[r] > TRI_WAVE) s_todo[atomicAdd(&s_ntodo, 1u)] = (int32_t)r;
    __syncthreads();
    const uint32_t ntodo = s_ntodo;
    for (uint32_t t = 0; t < ntodo; t++) {
      const int32_t a = s_todo[t];
      const int32_t sa = ptr[a], na = ptr[a + 1] - sa;
      uint64_t ha = 0;   // (the same in every lane of a wave)
      uint32_t looked = 0;
      for (int32_t c0 = 0; c0 < na; c0 += TRI_CHUNK) {
        const int32_t nc = min(TRI_CHUNK, na - c0);
        __syncthreads();   // (the chunk before this one is done with)
        for (int32_t i = (int32_t)threadIdx.x; i < nc; i += WL_BS) s_chunk[i] = col[sa + c0 + i];
        __syncthreads();
        for (int32_t i = wave; i < na; i += WL_BS / 64) {   // every b of the whole list, against this chunk
          const int32_t b = col[sa + i];
          const int32_t sb = ptr[b], lb = ptr[b + 1] - sb;
          const uint32_t hb = tri_stream<PER_VERTEX>(col, sb, lb, s_chunk, (uint32_t)nc, tri, &looked);
          if (PER_VERTEX && hb && lane == 0) tri_add(tri, b, hb);
          ha += hb;
        }
      }
      probes += looked;
      if (lane == 0) {
        if (PER_VERTEX && ha) tri_add(tri, a, ha);
        hits += ha;
        if (wave == 0) probes += (uint64_t)na;   // (staged once, chunk by chunk)
      }
    }
    __syncthreads();   // (s_todo and s_ntodo are done with)
  }
  hits = wl_block_fold<WlSum>(hits);
  probes = wl_block_fold<WlSum>(probes);
  if (threadIdx.x == 0) part[blockIdx.x] = TriPart{hits, probes};
}

// Closes the call: one workgroup sums the TriParts of the two counting launches.
__global__ __launch_bounds__(WL_BS) void tri_finish(TriCtl *ctl, int nparts, const TriPart *__restrict__ part) {
  uint64_t hits = 0, probes = 0;
  for (int i = (int)threadIdx.x; i < nparts; i += WL_BS) { hits += part[i].hits; probes += part[i].probes; }
  hits = wl_block_fold<WlSum>(hits);
  probes = wl_block_fold<WlSum>(probes);
  if (threadIdx.x == 0) { ctl->triangles = hits; ctl->probes = probes; }
}

} // namespace sh
