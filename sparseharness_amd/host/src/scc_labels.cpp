// scc_labels.cpp -- the strongly connected components of a CSR pattern on the host, as the gold for sh_scc on matrices
// too large for a Python reference: Tarjan's algorithm ("Depth-first search and linear graph algorithms", SIAM J. Comput.
// 1972), single-threaded and iterative (an explicit stack: a path of a million vertices must not overflow the call
// stack).  The edge rule and the labels are sh_scc's: entry (r, c) is the edge c -> r when 0 <= c < rows and its 32 value
// bits are not all zero; label[v] is the largest vertex index of v's component.  The components of a graph and of its
// transpose are the same, so the search runs along the rows as stored (r -> c) and needs no transpose.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "sh_host.h"

extern "C" int sh_scc_labels(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                             int32_t *label) {
  if (rows < 0 || nnz < 0 || !row_ptr || !label || (nnz > 0 && (!col_idx || !val)))
    return -1;
  const uint32_t *bits = (const uint32_t *)val;
  std::vector<int32_t> index(rows, -1), low(rows, 0), stack, next(rows, 0);
  std::vector<uint8_t> on_stack(rows, 0);
  std::vector<int32_t> path;   // the vertices whose rows are being walked
  int32_t counter = 0;
  for (int64_t root = 0; root < rows; root++) {
    if (index[root] != -1) continue;
    path.push_back((int32_t)root);
    index[root] = low[root] = counter++;
    next[root] = row_ptr[root];
    stack.push_back((int32_t)root);
    on_stack[root] = 1;
    while (!path.empty()) {
      const int32_t v = path.back();
      if (next[v] < row_ptr[v + 1]) {
        const int32_t j = next[v]++;
        const int32_t c = col_idx[j];
        if (c < 0 || (int64_t)c >= rows || bits[j] == 0u) continue;
        if (index[c] == -1) {
          index[c] = low[c] = counter++;
          next[c] = row_ptr[c];
          stack.push_back(c);
          on_stack[c] = 1;
          path.push_back(c);
        } else if (on_stack[c]) {
          low[v] = std::min(low[v], index[c]);
        }
        continue;
      }
      path.pop_back();
      if (!path.empty()) low[path.back()] = std::min(low[path.back()], low[v]);
      if (low[v] == index[v]) {   // v closes a component: what sits above it on the stack
        size_t at = stack.size();
        int32_t top = -1;
        do {
          at--;
          top = std::max(top, stack[at]);
        } while (stack[at] != v);
        for (size_t i = at; i < stack.size(); i++) { label[stack[i]] = top; on_stack[stack[i]] = 0; }
        stack.resize(at);
      }
    }
  }
  return 0;
}
