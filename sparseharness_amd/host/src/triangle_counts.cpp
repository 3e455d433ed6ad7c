// triangle_counts.cpp -- exact triangle counts per vertex on the host, single-threaded, as the gold for sh_tri on
// matrices too large for a Python reference and as the baseline of tools/tri_bench.py: clean, degree-orient, sort,
// merge-intersect (the forward algorithm: Schank, Wagner, WEA 2005; Latapy, TCS 2008).  The edge rule and the outputs
// are sh_tri's: entry (r, c) counts when 0 <= c < rows and its 32 value bits are not all zero; the graph is the simple
// undirected graph under those entries (no self-loops, no parallel edges); tri[v] is the number of triangles through v,
// deg[v] its degree.  The intersection is a two-pointer merge of two sorted lists: it shares no code with the device.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sh_host.h"

extern "C" int sh_triangle_counts(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                  uint64_t *tri, int32_t *deg) {
  if (rows < 0 || nnz < 0 || !row_ptr || !tri || !deg || (nnz > 0 && (!col_idx || !val)))
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
  for (int64_t v = 0; v < rows; v++) { tri[v] = 0; deg[v] = 0; }
  for (const auto &e : edges) { deg[e.first]++; deg[e.second]++; }
  // orient from the smaller (deg, index) to the larger; the lists come out ascending (the edges are sorted by both ends)
  const auto before = [&](int32_t u, int32_t v) { return deg[u] != deg[v] ? deg[u] < deg[v] : u < v; };
  std::vector<int64_t> start((size_t)rows + 1, 0);
  for (const auto &e : edges) start[(before(e.first, e.second) ? e.first : e.second) + 1]++;
  for (int64_t v = 0; v < rows; v++) start[v + 1] += start[v];
  std::vector<int32_t> fwd(edges.size());
  {
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (const auto &e : edges) {
      const bool f = before(e.first, e.second);
      fwd[at[f ? e.first : e.second]++] = f ? e.second : e.first;
    }
  }
  for (int64_t v = 0; v < rows; v++) std::sort(fwd.begin() + start[v], fwd.begin() + start[v + 1]);
  // merge-intersect N+(a) and N+(b) for every forward edge a -> b
  for (int64_t a = 0; a < rows; a++)
    for (int64_t i = start[a]; i < start[a + 1]; i++) {
      const int32_t b = fwd[i];
      int64_t p = start[a], q = start[b];
      const int64_t pe = start[a + 1], qe = start[b + 1];
      while (p < pe && q < qe) {
        if (fwd[p] < fwd[q]) p++;
        else if (fwd[q] < fwd[p]) q++;
        else { tri[a]++; tri[b]++; tri[fwd[p]]++; p++; q++; }
      }
    }
  return 0;
}
