// trsv_solve.cpp -- the sparse triangular solve on the host, single-threaded, as the gold for sh_trsv on matrices too large
// for a Python reference and as the baseline of tools/trsv_bench.py: the lists (a stable sort of the strictly-triangular
// entries by (row, column)), the diagonal, the levels, and plain substitution in the order of the rows.  The definition
// is sh_trsv's (include/sparseharness_hip.h): every stored entry with 0 <= c < rows takes part whatever its value, entries
// of the other triangle and columns out of range are ignored, the diagonal too when unit; d[r] = the diagonal entries of
// r widened to float64 and added left to right from +0.0; x[r] = (b[r] - S_r) / d[r] with S_r = SUM over r's list of
// (double)val_j * x[col_j].  SUM is float64 in the order the header fixes (pieces of 2048 entries, 64 strided partials
// each started from +0.0, a fixed butterfly, the piece sums left to right), restated here over plain arrays: it shares
// no code with the device.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "sh_host.h"

namespace {

constexpr int32_t PIECE = 2048;

// SUM of a list of signed terms: every partial starts from +0.0, so none is -0.0 and the padding is exact
template <class Term>
double pieces_sum(int64_t len, Term term) {
  double acc = 0.0;
  for (int64_t p0 = 0; p0 < len; p0 += PIECE) {
    const int64_t pe = std::min<int64_t>(len, p0 + PIECE);
    double partial[64];
    for (int l = 0; l < 64; l++) partial[l] = 0.0;
    for (int64_t j = p0; j < pe; j++) partial[(j - p0) & 63] = partial[(j - p0) & 63] + term(j);
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < 64; l++)
        if (!(l & o)) partial[l] = partial[l ^ o] = partial[l] + partial[l ^ o];
    acc = acc + partial[0];
  }
  return acc;
}
template <class Term>
double lane_sum(int64_t len, Term term) {   // len <= 8: the butterfly's levels 32, 16 and 8 add +0.0
  double t[8];
  for (int k = 0; k < 8; k++) t[k] = k < len ? 0.0 + term(k) : 0.0;
  return ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
}
template <class Term>
double list_sum(int64_t len, Term term) { return len <= 8 ? lane_sum(len, term) : pieces_sum(len, term); }

} // namespace

extern "C" double sh_trsv_list_sum(const double *t, int64_t n, int32_t tier) {
  const auto term = [&](int64_t j) { return t[j]; };
  if (tier == 1 && n <= 8) return lane_sum(n, term);
  if (tier == 2) return pieces_sum(n, term);
  return list_sum(n, term);
}

extern "C" int sh_trsv_solve(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val, const void *b,
                             int32_t uplo, int32_t unit, int32_t f32, void *x, int32_t *level_out, int64_t *figures) {
  if (rows < 0 || nnz < 0 || !row_ptr || (rows > 0 && (!b || !x)) || (nnz > 0 && (!col_idx || !val)) || (uplo != 0 && uplo != 1) ||
      (unit != 0 && unit != 1) || (f32 != 0 && f32 != 1))
    return -1;
  const float *a = (const float *)val;
  // the lists: per row the strictly-triangular entries, a stable sort by column keeps parallel entries in the order given
  std::vector<int64_t> ptr((size_t)rows + 1, 0);
  std::vector<int32_t> col;
  std::vector<float> lv;
  std::vector<double> d((size_t)rows, 0.0);
  std::vector<int32_t> at;
  int64_t max_list = 0, zero_diag = 0, first_zero = -1;
  for (int64_t r = 0; r < rows; r++) {
    at.clear();
    double sum = 0.0;
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const int32_t c = col_idx[j];
      if (c < 0 || (int64_t)c >= rows) continue;
      if ((int64_t)c == r) { sum = sum + (double)a[j]; continue; }
      if (uplo ? (int64_t)c > r : (int64_t)c < r) at.push_back(j);
    }
    std::stable_sort(at.begin(), at.end(), [&](int32_t p, int32_t q) { return col_idx[p] < col_idx[q]; });
    for (const int32_t j : at) { col.push_back(col_idx[j]); lv.push_back(a[j]); }
    ptr[r + 1] = (int64_t)col.size();
    max_list = std::max<int64_t>(max_list, (int64_t)at.size());
    if (!unit) {
      d[r] = sum;
      if (sum == 0.0) { zero_diag++; if (first_zero < 0) first_zero = r; }
    }
  }
  // substitution in the order of the rows (lower: ascending, upper: descending); a row's list is ready when it is reached
  std::vector<double> xs((size_t)rows);
  std::vector<int32_t> level((size_t)rows, 0);
  std::vector<int64_t> width;
  for (int64_t i = 0; i < rows; i++) {
    const int64_t r = uplo ? rows - 1 - i : i;
    const int64_t s = ptr[r], len = ptr[r + 1] - s;
    int32_t L = 0;
    for (int64_t j = s; j < s + len; j++) L = std::max(L, level[col[j]] + 1);
    level[r] = L;
    if ((int64_t)width.size() <= L) width.resize((size_t)L + 1, 0);
    width[L]++;
    const double S = list_sum(len, [&](int64_t k) { return (double)lv[s + k] * xs[col[s + k]]; });
    const double rhs = f32 ? (double)((const float *)b)[r] : ((const double *)b)[r];
    double v = rhs - S;
    if (!unit) v = v / d[r];
    xs[r] = v;
  }
  for (int64_t r = 0; r < rows; r++) {   // (b and x may be the same array: b has been read)
    if (f32) ((float *)x)[r] = (float)xs[r];
    else ((double *)x)[r] = xs[r];
  }
  if (level_out && rows > 0) memcpy(level_out, level.data(), (size_t)rows * 4);
  if (figures) {
    figures[0] = (int64_t)col.size();
    figures[1] = (int64_t)width.size();
    figures[2] = max_list;
    figures[3] = width.empty() ? 0 : *std::max_element(width.begin(), width.end());
    figures[4] = zero_diag;
    figures[5] = first_zero;
  }
  return 0;
}
