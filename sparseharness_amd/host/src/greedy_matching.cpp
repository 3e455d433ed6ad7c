// greedy_matching.cpp -- the greedy weighted matching of the simple undirected graph under a square CSR matrix, the
// float32 values as weights, on the host, single-threaded, as the gold for sh_match on matrices too large for a Python
// reference and as the baseline of tools/match_bench.py: clean (und_edges.h, shared with msf_edges.cpp), sort the edges
// by MKEY, take them in that order and keep an edge when both its ends are still free.  The edge rule and the weight rule
// are sh_msf's; MKEY(e) = hi << 32 | lo with hi = k(weight[e]) for heavy == 0 and ~k(weight[e]) for heavy == 1, lo = e
// for seed == 0 and mix32(e ^ seed) otherwise.  This is the definition: it knows nothing of rounds, bids or dominant
// edges, and shares no code with the device, which never sorts.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sh_host.h"
#include "und_edges.h"

extern "C" int sh_greedy_matching(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                  int32_t heavy, uint32_t seed, int32_t *edge_u, int32_t *edge_v, uint32_t *weight,
                                  int32_t *in_match, int32_t *mate, int64_t *edges_out, int64_t *pairs_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !edges_out || (heavy != 0 && heavy != 1) ||
      (nnz > 0 && (!col_idx || !val || !edge_u || !edge_v || !weight || !in_match)) || (rows > 0 && !mate))
    return -1;
  std::vector<uint32_t> wk;
  const int64_t M = sh_host::weighted_edges(rows, nnz, row_ptr, col_idx, (const uint32_t *)val, edge_u, edge_v, weight, wk);
  *edges_out = M;
  // (MKEY, e): lo is a bijection of e, so the keys alone order the edges; e rides along to save inverting mix32
  std::vector<std::pair<uint64_t, int64_t>> order((size_t)M);
  for (int64_t e = 0; e < M; e++) {
    const uint32_t hi = heavy ? ~wk[e] : wk[e];
    const uint32_t lo = seed == 0u ? (uint32_t)e : sh_host::mix32((uint32_t)e ^ seed);
    order[e] = {((uint64_t)hi << 32) | lo, e};
    in_match[e] = 0;
  }
  std::sort(order.begin(), order.end());
  for (int64_t v = 0; v < rows; v++) mate[v] = -1;
  int64_t pairs = 0;
  for (const auto &ke : order) {
    const int64_t e = ke.second;
    const int32_t u = edge_u[e], v = edge_v[e];
    if (mate[u] >= 0 || mate[v] >= 0) continue;
    mate[u] = v;
    mate[v] = u;
    in_match[e] = 1;
    pairs++;
  }
  if (pairs_out) *pairs_out = pairs;
  return 0;
}
