// msf_edges.cpp -- the minimum spanning forest of the simple undirected graph under a square CSR matrix, the float32
// values as weights, on the host, single-threaded, as the gold for sh_msf on matrices too large for a Python reference and
// as the baseline of tools/msf_bench.py: clean, sort the keys, then Kruskal's loop with a union-find.  The edge rule, the
// weight rule and the outputs are sh_msf's: entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not
// all zero; edge e is the e-th smallest pair u < v; weights are compared by k(b) = b ^ 0xFFFFFFFF if the sign bit of the
// bits b is set, else b ^ 0x80000000; the weight of an edge is the smallest, by k, over all counting entries (u, v) and
// (v, u); KEY(e) = k(weight[e]) << 32 | e, and the forest is what Kruskal's algorithm returns when it takes the edges in
// ascending KEY.  It shares no code with the device, which never sorts by weight and grows all trees at once.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "sh_host.h"
#include "und_edges.h"

extern "C" int sh_msf_edges(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                            int32_t *edge_u, int32_t *edge_v, uint32_t *weight, int32_t *in_msf, int32_t *comp,
                            int64_t *edges_out, int64_t *components_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !edges_out || (nnz > 0 && (!col_idx || !val || !edge_u || !edge_v || !weight || !in_msf)) ||
      (rows > 0 && !comp))
    return -1;
  // clean (und_edges.h): the edges, their ends, weights and k(weight)
  std::vector<uint32_t> wk;
  const int64_t M = sh_host::weighted_edges(rows, nnz, row_ptr, col_idx, (const uint32_t *)val, edge_u, edge_v, weight, wk);
  std::vector<uint64_t> keys((size_t)M);
  for (int64_t e = 0; e < M; e++) {
    in_msf[e] = 0;
    keys[e] = ((uint64_t)wk[e] << 32) | (uint64_t)e;
  }
  *edges_out = M;
  std::sort(keys.begin(), keys.end());
  // Kruskal: union by size, path halving
  std::vector<int32_t> parent((size_t)rows), size((size_t)rows, 1);
  std::iota(parent.begin(), parent.end(), 0);
  const auto find = [&](int32_t v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
  };
  int64_t components = rows;
  for (const uint64_t key : keys) {
    const int64_t e = (int64_t)(key & 0xFFFFFFFFull);
    int32_t a = find(edge_u[e]), b = find(edge_v[e]);
    if (a == b) continue;
    if (size[a] < size[b]) std::swap(a, b);
    parent[b] = a;
    size[a] += size[b];
    in_msf[e] = 1;
    components--;
  }
  if (components_out) *components_out = components;
  // comp[v] = the largest index of v's component
  std::vector<int32_t> top((size_t)rows, -1);
  for (int64_t v = 0; v < rows; v++) {
    const int32_t r = find((int32_t)v);
    top[r] = std::max(top[r], (int32_t)v);
  }
  for (int64_t v = 0; v < rows; v++) comp[v] = top[find((int32_t)v)];
  return 0;
}
