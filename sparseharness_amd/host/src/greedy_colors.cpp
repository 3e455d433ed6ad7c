// greedy_colors.cpp -- the first-fit colouring of the simple undirected graph under a square CSR pattern in a fixed
// priority order, on the host, single-threaded, as the gold for sh_color on matrices too large for a Python reference and
// as the baseline of tools/color_bench.py: clean, sort the vertices by their keys, then one serial loop over them in that
// order, each taking the smallest colour that none of its coloured neighbours holds.  The edge rule, the order and the
// outputs are sh_color's: entry (r, c) counts when 0 <= c < rows and its 32 value bits are not all zero; the graph is the
// simple undirected graph under those entries (no self-loops, no parallel edges); v precedes u when (primary(v), tie(v))
// > (primary(u), tie(u)), primary = prio[v] when prio is given, else deg[v] for order 2, else 0, tie = the smaller index
// first for order 0 and the larger mix32(v ^ seed) first otherwise.  depth[v] is the number of vertices on the longest
// chain of preceding neighbours that ends in v, counted from 0: the round in which sh_color colours v.  It shares no
// code with the device, which colours a whole depth per round and never sorts.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sh_host.h"
#include "und_edges.h"

using sh_host::mix32;

extern "C" int sh_greedy_colors(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                int32_t order, uint32_t seed, const int32_t *prio, int32_t *color, int32_t *depth,
                                int32_t *colors_out, int64_t *edges_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !color || !depth || order < 0 || order > 2 || (nnz > 0 && (!col_idx || !val)))
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
  std::vector<int32_t> deg((size_t)rows, 0);
  for (const auto &e : edges) { deg[e.first]++; deg[e.second]++; }
  // the neighbour lists
  std::vector<int64_t> start((size_t)rows + 1, 0);
  for (int64_t v = 0; v < rows; v++) start[v + 1] = start[v] + deg[v];
  std::vector<int32_t> nb(2 * edges.size());
  {
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (const auto &e : edges) { nb[at[e.first]++] = e.second; nb[at[e.second]++] = e.first; }
  }
  // the vertices in the order: the larger (primary, tie) first
  struct Key { int32_t primary; uint32_t tie; int32_t v; };
  std::vector<Key> seq((size_t)rows);
  for (int64_t v = 0; v < rows; v++) {
    const int32_t primary = prio ? prio[v] : order == 2 ? deg[v] : 0;
    const uint32_t tie = order == 0 ? 0xFFFFFFFFu - (uint32_t)v : mix32((uint32_t)v ^ seed);
    seq[v] = Key{primary, tie, (int32_t)v};
  }
  std::sort(seq.begin(), seq.end(), [](const Key &a, const Key &b) {
    return a.primary != b.primary ? a.primary > b.primary : a.tie > b.tie;
  });
  // first-fit in that order; mark[c] == v + 1: colour c is held by a coloured neighbour of v
  for (int64_t v = 0; v < rows; v++) { color[v] = -1; depth[v] = 0; }
  int32_t md = 0;
  for (int64_t v = 0; v < rows; v++) md = std::max(md, deg[v]);
  std::vector<int32_t> mark((size_t)md + 2, 0);
  int32_t colors = 0;
  for (const Key &k : seq) {
    const int32_t v = k.v;
    int32_t d = 0;
    for (int64_t j = start[v]; j < start[v + 1]; j++) {
      const int32_t u = nb[j];
      if (color[u] < 0) continue;   // v precedes u
      if (color[u] <= md) mark[color[u]] = v + 1;
      d = std::max(d, depth[u] + 1);
    }
    int32_t c = 0;
    while (mark[c] == v + 1) c++;   // (at most deg[v] marks: ends by deg[v] <= md, and mark[md + 1] is never set)
    color[v] = c;
    depth[v] = d;
    colors = std::max(colors, c + 1);
  }
  if (colors_out) *colors_out = colors;
  return 0;
}
