// ilu0_factor.cpp -- the incomplete LU factorisation without fill on the host, single-threaded, as the gold for sh_ilu0 on
// matrices too large for a Python reference and as the baseline of tools/ilu0_bench.py.  The definition is sh_ilu0's
// (include/sparseharness_hip.h): the slots of row r are the distinct columns 0 <= c < rows among its entries in ascending
// c; a[r, c] = the entries (r, c) in the order given, widened to float64 and added left to right from +0.0; then the
// row-wise IKJ recurrence in float64, the rows in ascending order, every product rounded once and the subtraction a second
// rounding (this file is compiled with -ffp-contract=off).  It shares no code with the device: the slot (r, j) of an
// update is found through a dense map of row r's columns, not by bisection.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sh_host.h"

extern "C" int sh_ilu0_factor(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val, int32_t f32,
                              void *lu, int32_t *level_out, int64_t *figures) {
  if (rows < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!col_idx || !val || !lu)) || (f32 != 0 && f32 != 1))
    return -1;
  const float *a = (const float *)val;
  // the slots: per row a stable sort of the entries inside the matrix by column; the first of every run is the head
  std::vector<int64_t> ptr((size_t)rows + 1, 0);
  std::vector<int32_t> col, head;          // per slot: its column, the position of its first entry
  std::vector<double> w;                   // per slot: a[r, c], then the factor
  std::vector<int64_t> dslot((size_t)rows, -1), up((size_t)rows, 0);
  std::vector<int32_t> at;
  int64_t max_list = 0, missing = 0, first_missing = -1;
  for (int64_t r = 0; r < rows; r++) {
    at.clear();
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++)
      if (col_idx[j] >= 0 && (int64_t)col_idx[j] < rows) at.push_back(j);
    std::stable_sort(at.begin(), at.end(), [&](int32_t p, int32_t q) { return col_idx[p] < col_idx[q]; });
    for (size_t i = 0; i < at.size(); i++) {
      const int32_t j = at[i];
      if (i == 0 || col_idx[j] != col_idx[at[i - 1]]) {
        col.push_back(col_idx[j]);
        head.push_back(j);
        w.push_back(0.0);
      }
      w.back() = w.back() + (double)a[j];
    }
    ptr[r + 1] = (int64_t)col.size();
    max_list = std::max(max_list, ptr[r + 1] - ptr[r]);
    up[r] = ptr[r + 1];
    for (int64_t s = ptr[r]; s < ptr[r + 1]; s++) {
      if ((int64_t)col[s] == r) dslot[r] = s;
      if ((int64_t)col[s] > r) { up[r] = s; break; }
    }
    if (dslot[r] < 0) { missing++; if (first_missing < 0) first_missing = r; }
  }
  // the recurrence, the rows in ascending order: every row k < r is final when row r is reached
  std::vector<int64_t> where((size_t)rows, -1);   // the slot of column j in the row at hand
  std::vector<int32_t> level((size_t)rows, 0);
  std::vector<int64_t> width;
  int64_t work = 0, zero_pivots = 0, first_zero = -1;
  for (int64_t r = 0; r < rows; r++) {
    for (int64_t s = ptr[r]; s < ptr[r + 1]; s++) where[col[s]] = s;
    int32_t L = 0;
    for (int64_t s = ptr[r]; s < ptr[r + 1] && (int64_t)col[s] < r; s++) {
      const int64_t k = col[s];
      L = std::max(L, level[k] + 1);
      const double piv = dslot[k] >= 0 ? w[dslot[k]] : 0.0;
      const double wk = w[s] / piv;
      w[s] = wk;
      work += ptr[k + 1] - up[k];
      for (int64_t t = up[k]; t < ptr[k + 1]; t++) {
        const int64_t q = where[col[t]];
        if (q < 0) continue;
        const double p = wk * w[t];
        w[q] = w[q] - p;
      }
    }
    for (int64_t s = ptr[r]; s < ptr[r + 1]; s++) where[col[s]] = -1;
    level[r] = L;
    if ((int64_t)width.size() <= L) width.resize((size_t)L + 1, 0);
    width[L]++;
    const double piv = dslot[r] >= 0 ? w[dslot[r]] : 0.0;
    if (piv == 0.0) { zero_pivots++; if (first_zero < 0) first_zero = r; }
  }
  // lu in the positions of the entries: the slot's value at its head, +0.0 everywhere else
  for (int64_t j = 0; j < nnz; j++) {
    if (f32) ((float *)lu)[j] = 0.0f;
    else ((double *)lu)[j] = 0.0;
  }
  for (size_t s = 0; s < col.size(); s++) {
    if (f32) ((float *)lu)[head[s]] = (float)w[s];
    else ((double *)lu)[head[s]] = w[s];
  }
  if (level_out && rows > 0) memcpy(level_out, level.data(), (size_t)rows * 4);
  if (figures) {
    figures[0] = (int64_t)col.size();
    figures[1] = (int64_t)width.size();
    figures[2] = max_list;
    figures[3] = width.empty() ? 0 : *std::max_element(width.begin(), width.end());
    figures[4] = missing;
    figures[5] = first_missing;
    figures[6] = work;
    figures[7] = zero_pivots;
    figures[8] = first_zero;
  }
  return 0;
}
