// wcc_labels.cpp -- the weakly connected components of a CSR pattern on the host, as the gold for sh_wcc on matrices too
// large for a Python reference: a single-threaded union-find (Tarjan, "Efficiency of a good but not linear set union
// algorithm", J. ACM 1975) that links the smaller root under the larger, so that a root is the largest index of its set,
// with path halving in the search.  The edge rule and the labels are sh_wcc's: entry (r, c) joins r and c when
// 0 <= c < rows and its 32 value bits are not all zero, whatever its direction; label[v] is the largest vertex index of
// v's component.
#include <cstdint>
#include <vector>

#include "sh_host.h"

extern "C" int sh_wcc_labels(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                             int32_t *label) {
  if (rows < 0 || nnz < 0 || !row_ptr || !label || (nnz > 0 && (!col_idx || !val)))
    return -1;
  const uint32_t *bits = (const uint32_t *)val;
  std::vector<int32_t> parent(rows);
  for (int64_t v = 0; v < rows; v++) parent[v] = (int32_t)v;
  const auto find = [&](int32_t v) {
    while (parent[v] != v) {
      parent[v] = parent[parent[v]];   // path halving
      v = parent[v];
    }
    return v;
  };
  for (int64_t r = 0; r < rows; r++)
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const int32_t c = col_idx[j];
      if (c < 0 || (int64_t)c >= rows || bits[j] == 0u) continue;
      const int32_t a = find((int32_t)r), b = find(c);
      if (a < b) parent[a] = b;
      else if (b < a) parent[b] = a;
    }
  for (int64_t v = 0; v < rows; v++) label[v] = find((int32_t)v);
  return 0;
}
