// truss_numbers.cpp -- the support and the truss number of every edge on the host, single-threaded, as the gold for
// sh_truss on matrices too large for a Python reference and as the baseline of tools/truss_bench.py: clean, count the
// triangles through every edge, then the bucket algorithm of Wang and Cheng ("Truss decomposition in massive networks",
// VLDB 2012): the edges leave one at a time in the order of their remaining support.  The edge rule and the outputs are
// sh_truss's: entry (r, c) counts when 0 <= c < rows and its 32 value bits are not all zero; the graph is the simple
// undirected graph under those entries (no self-loops, no parallel edges); edge e is the e-th smallest pair (u, v),
// u < v; support[e] = |N(u) & N(v)|; truss[e] is the largest k such that e lies in a subgraph all of whose edges are in
// at least k - 2 triangles of it (Cohen's convention: 2 for an edge in no triangle).  It shares no code with the device,
// which peels whole levels in rounds.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sh_host.h"

namespace {

struct Lists {
  std::vector<int64_t> start;
  std::vector<int32_t> nb, id;   // the neighbours of every vertex, ascending, and the edge each entry stands for
  // the entry of w in v's list, or -1
  int64_t find(int32_t v, int32_t w) const {
    const int32_t *b = nb.data() + start[v], *e = nb.data() + start[v + 1];
    const int32_t *p = std::lower_bound(b, e, w);
    return (p != e && *p == w) ? (int64_t)(p - nb.data()) : -1;
  }
};

} // namespace

extern "C" int sh_truss_numbers(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                int32_t *edge_u, int32_t *edge_v, int32_t *support, int32_t *truss, int64_t *edges_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !edges_out || (nnz > 0 && (!col_idx || !val || !edge_u || !edge_v || !support || !truss)))
    return -1;
  const uint32_t *bits = (const uint32_t *)val;
  // clean: every entry that counts, as (smaller, larger), once; the sorted order is the order of the edge ids
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
  const int64_t M = (int64_t)edges.size();
  *edges_out = M;
  if (M == 0)
    return 0;
  // the neighbour lists (ascending: the edges are sorted, and every list gets its smaller neighbours before its larger)
  Lists L;
  L.start.assign((size_t)rows + 1, 0);
  for (const auto &e : edges) { L.start[e.first + 1]++; L.start[e.second + 1]++; }
  for (int64_t v = 0; v < rows; v++) L.start[v + 1] += L.start[v];
  L.nb.resize(2 * (size_t)M);
  L.id.resize(2 * (size_t)M);
  {
    std::vector<int64_t> at(L.start.begin(), L.start.end() - 1);
    for (int64_t i = 0; i < M; i++) {   // (u, v) ascending by u then v: v's list gets its u's in ascending order ...
      const int32_t u = edges[i].first, v = edges[i].second;
      L.nb[at[v]] = u; L.id[at[v]++] = (int32_t)i;
    }
    for (int64_t i = 0; i < M; i++) {   // ... and after them u's list its v's
      const int32_t u = edges[i].first, v = edges[i].second;
      L.nb[at[u]] = v; L.id[at[u]++] = (int32_t)i;
    }
  }
  // for every w common to the two ends of e (the shorter list walked, the longer one searched): f(edge a-w, edge b-w)
  const auto common = [&](int64_t e, auto f) {
    int32_t a = edges[e].first, b = edges[e].second;
    if (L.start[b + 1] - L.start[b] < L.start[a + 1] - L.start[a]) std::swap(a, b);
    for (int64_t j = L.start[a]; j < L.start[a + 1]; j++) {
      const int64_t j2 = L.find(b, L.nb[j]);
      if (j2 >= 0) f(L.id[j], L.id[j2]);
    }
  };
  int32_t ms = 0;
  for (int64_t e = 0; e < M; e++) {
    edge_u[e] = edges[e].first;
    edge_v[e] = edges[e].second;
    int32_t n = 0;
    common(e, [&](int32_t, int32_t) { n++; });
    support[e] = n;
    ms = std::max(ms, n);
  }
  // order: the edges ascending by remaining support; bin[s]: where those of support s begin in it; pos: its inverse
  std::vector<int32_t> sup(support, support + M);
  std::vector<int64_t> bin((size_t)ms + 2, 0);
  for (int64_t e = 0; e < M; e++) bin[sup[e] + 1]++;
  for (int32_t s = 0; s <= ms; s++) bin[s + 1] += bin[s];
  std::vector<int32_t> order((size_t)M);
  std::vector<int64_t> pos((size_t)M);
  {
    std::vector<int64_t> at(bin.begin(), bin.end() - 1);
    for (int64_t e = 0; e < M; e++) { pos[e] = at[sup[e]]++; order[pos[e]] = (int32_t)e; }
  }
  std::vector<char> gone((size_t)M, 0);
  for (int64_t i = 0; i < M; i++) {
    const int32_t e = order[i];   // leaves now: sup[e] is final
    truss[e] = sup[e] + 2;
    gone[e] = 1;
    common(e, [&](int32_t e1, int32_t e2) {
      if (gone[e1] || gone[e2]) return;   // the triangle was taken apart before
      for (const int32_t x : {e1, e2}) {
        if (sup[x] <= sup[e]) continue;
        // x moves to the front of its bin, and the bin starts one later: one triangle less
        const int32_t sx = sup[x];
        const int64_t px = pos[x], pw = bin[sx];
        const int32_t w = order[pw];
        if (x != w) { pos[x] = pw; order[px] = w; pos[w] = px; order[pw] = x; }
        bin[sx]++;
        sup[x]--;
      }
    });
  }
  return 0;
}
