// core_numbers.cpp -- the core number of every vertex on the host, single-threaded, as the gold for sh_core on matrices
// too large for a Python reference and as the baseline of tools/core_bench.py: clean, then the bucket algorithm of
// Batagelj and Zaversnik ("An O(m) algorithm for cores decomposition of networks", 2003), O(n + M) after the clean-up's
// sort.  The edge rule and the outputs are sh_core's: entry (r, c) counts when 0 <= c < rows and its 32 value bits are
// not all zero; the graph is the simple undirected graph under those entries (no self-loops, no parallel edges);
// core[v] is the largest k such that v lies in a subgraph whose vertices all have at least k neighbours in it, deg[v]
// the degree.  Vertices leave one at a time in the order of their remaining degree: it shares no code with the device,
// which peels whole levels in rounds.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sh_host.h"

extern "C" int sh_core_numbers(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                               int32_t *core, int32_t *deg, int64_t *edges_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !core || !deg || (nnz > 0 && (!col_idx || !val)))
    return -1;
  const uint32_t *bits = (const uint32_t *)val;
  // clean: every entry that counts, as (smaller, larger), once
  std::vector<std::pair<int32_t, int32_t>> edges;
  edges.reserve((size_t)nnz);
  for (int64_t r = 0; r < rows; r++)
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const int32_t c = col_idx[j];
      if (c < 0 || (int64_t)c >= rows || bits[j] == 0u || (int64_t)c == r) continue;
      edges.emplace_back(std::min((int32_t)r, c), std::max((int32_t)r, c));
    }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  if (edges_out) *edges_out = (int64_t)edges.size();
  for (int64_t v = 0; v < rows; v++) deg[v] = 0;
  for (const auto &e : edges) { deg[e.first]++; deg[e.second]++; }
  // the neighbour lists
  std::vector<int64_t> start((size_t)rows + 1, 0);
  for (int64_t v = 0; v < rows; v++) start[v + 1] = start[v] + deg[v];
  std::vector<int32_t> nb(2 * edges.size());
  {
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (const auto &e : edges) { nb[at[e.first]++] = e.second; nb[at[e.second]++] = e.first; }
  }
  // vert: the vertices ascending by remaining degree; bin[d]: where the vertices of degree d begin in it; pos: its inverse
  int32_t md = 0;
  for (int64_t v = 0; v < rows; v++) md = std::max(md, deg[v]);
  std::vector<int64_t> bin((size_t)md + 2, 0);
  for (int64_t v = 0; v < rows; v++) bin[deg[v] + 1]++;
  for (int32_t d = 0; d <= md; d++) bin[d + 1] += bin[d];
  std::vector<int32_t> vert((size_t)rows);
  std::vector<int64_t> pos((size_t)rows);
  {
    std::vector<int64_t> at(bin.begin(), bin.end() - 1);
    for (int64_t v = 0; v < rows; v++) { pos[v] = at[deg[v]]++; vert[pos[v]] = (int32_t)v; }
  }
  for (int64_t v = 0; v < rows; v++) core[v] = deg[v];
  for (int64_t i = 0; i < rows; i++) {
    const int32_t v = vert[i];   // leaves now: core[v] is final
    for (int64_t j = start[v]; j < start[v + 1]; j++) {
      const int32_t u = nb[j];
      if (core[u] <= core[v]) continue;
      // u moves to the front of its bin, and the bin starts one later: one degree less
      const int32_t du = core[u];
      const int64_t pu = pos[u], pw = bin[du];
      const int32_t w = vert[pw];
      if (u != w) { pos[u] = pw; vert[pu] = w; pos[w] = pu; vert[pw] = u; }
      bin[du]++;
      core[u]--;
    }
  }
  return 0;
}
