/* und_edges.h -- what the host golds of the weighted undirected entry points (sh_msf: src/msf_edges.cpp; sh_match:
 * src/greedy_matching.cpp) and of sh_color (src/greedy_colors.cpp) share: the total order of float32 bit patterns, the
 * mixing bijection of the tie-breaks, and the weighted edge list of the simple undirected graph under a square CSR matrix.
 * Host code only; it shares no line with the device. */
#ifndef SH_UND_EDGES_H_
#define SH_UND_EDGES_H_
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sh_host {

/* k(b) = b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000, and its inverse */
inline uint32_t order_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u); }
inline uint32_t order_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

/* the bijection of the 32-bit words that sh_color and sh_match break ties with */
inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

/* Clean: every entry (r, c) that counts (0 <= c < rows, c != r, its 32 value bits not all zero) as ((smaller, larger),
 * k(value)); sorted, the first of a run is the edge with its smallest key.  Edge e is the e-th smallest pair u < v:
 * edge_u[e], edge_v[e], weight[e] (the 32 bits of the chosen entry) are written (nnz words suffice), and wk[e] =
 * k(weight[e]) for every e.  Returns M. */
inline int64_t weighted_edges(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const uint32_t *bits,
                              int32_t *edge_u, int32_t *edge_v, uint32_t *weight, std::vector<uint32_t> &wk) {
  struct Entry { uint64_t pair; uint32_t k; };
  std::vector<Entry> entries;
  entries.reserve((size_t)nnz);
  for (int64_t r = 0; r < rows; r++)
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const int32_t c = col_idx[j];
      if (c < 0 || (int64_t)c >= rows || bits[j] == 0u || (int64_t)c == r) continue;
      const uint64_t lo = (uint64_t)std::min<int64_t>(r, c), hi = (uint64_t)std::max<int64_t>(r, c);
      entries.push_back(Entry{(lo << 32) | hi, order_key(bits[j])});
    }
  std::sort(entries.begin(), entries.end(),
            [](const Entry &a, const Entry &b) { return a.pair != b.pair ? a.pair < b.pair : a.k < b.k; });
  int64_t M = 0;
  wk.clear();
  wk.reserve(entries.size());
  for (size_t i = 0; i < entries.size(); i++) {
    if (i > 0 && entries[i].pair == entries[i - 1].pair) continue;
    edge_u[M] = (int32_t)(entries[i].pair >> 32);
    edge_v[M] = (int32_t)(entries[i].pair & 0xFFFFFFFFull);
    weight[M] = order_bits(entries[i].k);
    wk.push_back(entries[i].k);
    M++;
  }
  return M;
}

}  // namespace sh_host
#endif /* SH_UND_EDGES_H_ */
