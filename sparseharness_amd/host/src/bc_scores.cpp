// bc_scores.cpp -- betweenness centrality on the host, single-threaded, as the gold for sh_bc on matrices too large for a
// Python reference and as the baseline of tools/bc_bench.py: clean (sort the entries that count, drop duplicates and
// self-loops), then Brandes' two sweeps per source (Brandes, J. Math. Sociol. 2001) with one queue.  The edge rule and
// the outputs are sh_bc's: entry (r, c) is the edge c -> r when 0 <= c < rows, c != r and its 32 value bits are not all
// zero; the graph is the simple directed graph under those entries.  Every sum is float64 and runs in the order that
// include/sparseharness_hip.h fixes (SUM: pieces of 2048 entries, 64 strided partials, a fixed butterfly, the piece sums
// left to right), restated here over plain arrays: it shares no code with the device.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "sh_host.h"

namespace {

constexpr int32_t PIECE = 2048;

// SUM over the entries [s, s + len) of a list, term(j) being +0.0 where entry j does not take part
template <class Term>
double list_sum(int64_t s, int64_t len, Term term) {
  if (len <= 8) {   // the butterfly's levels 32, 16 and 8 add +0.0
    double t[8];
    for (int k = 0; k < 8; k++) t[k] = k < len ? term(s + k) : 0.0;
    return ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
  }
  double acc = 0.0;
  for (int64_t p0 = 0; p0 < len; p0 += PIECE) {
    const int64_t pe = std::min<int64_t>(len, p0 + PIECE);
    double partial[64];
    for (int l = 0; l < 64; l++) partial[l] = 0.0;
    for (int64_t j = p0; j < pe; j++) partial[(j - p0) & 63] = partial[(j - p0) & 63] + term(s + j);
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < 64; l++)
        if (!(l & o)) partial[l] = partial[l ^ o] = partial[l] + partial[l ^ o];
    acc = acc + partial[0];
  }
  return acc;
}

} // namespace

extern "C" int sh_bc_scores(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                            const int32_t *sources, int32_t n_sources, int32_t accumulate, double *bc, double *sigma_out,
                            int32_t *level_out, int32_t *depth, int64_t *reached, double *sigma_max, int64_t *edges) {
  if (rows < 0 || nnz < 0 || n_sources < 0 || !row_ptr || (rows > 0 && !bc) || (nnz > 0 && (!col_idx || !val)) ||
      (n_sources > 0 && !sources) || (accumulate != 0 && accumulate != 1))
    return -1;
  for (int32_t i = 0; i < n_sources; i++)
    if (sources[i] < 0 || (int64_t)sources[i] >= rows) return -1;
  const uint32_t *bits = (const uint32_t *)val;
  // clean: every entry that counts, as (target, source), once; in_col comes out ascending, out_col after the second sort
  std::vector<std::pair<int32_t, int32_t>> in_e;
  in_e.reserve((size_t)nnz);
  for (int64_t r = 0; r < rows; r++)
    for (int32_t j = row_ptr[r]; j < row_ptr[r + 1]; j++) {
      const int32_t c = col_idx[j];
      if (c < 0 || (int64_t)c >= rows || bits[j] == 0u || (int64_t)c == r) continue;
      in_e.emplace_back((int32_t)r, c);
    }
  std::sort(in_e.begin(), in_e.end());
  in_e.erase(std::unique(in_e.begin(), in_e.end()), in_e.end());
  const size_t M = in_e.size();
  std::vector<std::pair<int32_t, int32_t>> out_e(M);
  for (size_t i = 0; i < M; i++) out_e[i] = {in_e[i].second, in_e[i].first};
  std::sort(out_e.begin(), out_e.end());
  std::vector<int64_t> in_ptr((size_t)rows + 1, 0), out_ptr((size_t)rows + 1, 0);
  std::vector<int32_t> in_col(M), out_col(M);
  for (size_t i = 0; i < M; i++) {
    in_ptr[in_e[i].first + 1]++; in_col[i] = in_e[i].second;
    out_ptr[out_e[i].first + 1]++; out_col[i] = out_e[i].second;
  }
  for (int64_t v = 0; v < rows; v++) { in_ptr[v + 1] += in_ptr[v]; out_ptr[v + 1] += out_ptr[v]; }
  if (!accumulate)
    for (int64_t v = 0; v < rows; v++) bc[v] = 0.0;
  std::vector<int32_t> level((size_t)rows), order((size_t)rows);
  std::vector<double> sigma((size_t)rows), delta((size_t)rows);
  std::vector<int64_t> lstart;
  std::fill(level.begin(), level.end(), -1);
  std::fill(sigma.begin(), sigma.end(), 0.0);
  std::fill(delta.begin(), delta.end(), 0.0);
  int64_t touched = 0;   // order[0, touched): the vertices the source before reached, the only ones whose state it changed
  for (int32_t i = 0; i < n_sources; i++) {
    const int32_t src = sources[i];
    for (int64_t k = 0; k < touched; k++) { level[order[k]] = -1; sigma[order[k]] = 0.0; delta[order[k]] = 0.0; }
    level[src] = 0; sigma[src] = 1.0; order[0] = src;
    lstart.assign({0, 1});
    int64_t walked = 0;
    double top = 1.0;
    int32_t L = 0;
    for (;; L++) {   // the forward sweep: level L = order[lstart[L], lstart[L + 1])
      const int64_t a = lstart[L], b = lstart[L + 1];
      int64_t tail = b;
      for (int64_t k = a; k < b; k++) {
        const int32_t v = order[k];
        walked += out_ptr[v + 1] - out_ptr[v];
        for (int64_t j = out_ptr[v]; j < out_ptr[v + 1]; j++) {
          const int32_t w = out_col[j];
          if (level[w] < 0) { level[w] = L + 1; order[tail++] = w; }
        }
      }
      if (tail == b) break;
      for (int64_t k = b; k < tail; k++) {
        const int32_t w = order[k];
        sigma[w] = list_sum(in_ptr[w], in_ptr[w + 1] - in_ptr[w], [&](int64_t j) {
          const int32_t v = in_col[j];
          return level[v] == L ? sigma[v] : 0.0;
        });
        top = std::max(top, sigma[w]);
      }
      lstart.push_back(tail);
    }
    for (int32_t B = L - 1; B >= 1; B--)   // the backward sweep (level 0 is the source alone)
      for (int64_t k = lstart[B]; k < lstart[B + 1]; k++) {
        const int32_t v = order[k];
        const double sv = sigma[v];
        delta[v] = list_sum(out_ptr[v], out_ptr[v + 1] - out_ptr[v], [&](int64_t j) {
          const int32_t w = out_col[j];
          return level[w] == B + 1 ? (sv / sigma[w]) * (1.0 + delta[w]) : 0.0;
        });
        bc[v] = bc[v] + delta[v];
      }
    if (depth) depth[i] = L;
    touched = lstart[L + 1];
    if (reached) reached[i] = touched;
    if (sigma_max) sigma_max[i] = top;
    if (edges) edges[i] = walked;
  }
  if (n_sources > 0) {
    if (sigma_out) memcpy(sigma_out, sigma.data(), (size_t)rows * 8);
    if (level_out) memcpy(level_out, level.data(), (size_t)rows * 4);
  }
  return 0;
}
