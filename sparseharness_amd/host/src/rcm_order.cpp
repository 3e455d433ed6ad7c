// rcm_order.cpp -- the reverse Cuthill-McKee ordering of the simple undirected graph under a square CSR pattern, on the
// host, single-threaded, as the gold for sh_rcm on matrices too large for a Python reference and as the baseline of
// tools/rcm_bench.py.  It is the serial definition itself: clean, sort every list by (deg, index), walk the vertices in
// ascending (deg, index); for every vertex v without a position pick the root by George and Liu's sweeps with a cap
// (r = v; a breadth-first search from r; at most `sweeps` times: x = the smallest vertex of the last level, stop if
// x == r, search from x, take x when its eccentricity is larger, otherwise stop), then number the component from r with
// one queue, appending each vertex's neighbours without a position in list order.  It shares no code with the device,
// which works over sorted labels, level by level, and never keeps a queue of its own.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "sh_host.h"

extern "C" int sh_rcm_order(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                            int32_t sweeps, int32_t reverse, int32_t *perm, int32_t *pos_out, int32_t *level_out,
                            int64_t *bandwidth, int64_t *profile, int32_t *components_out, int32_t *sweeps_out,
                            int64_t *edges_out, int64_t steps_cap, int32_t *kind, int64_t *size, int64_t *looked,
                            int64_t *steps_out) {
  if (rows < 0 || nnz < 0 || !row_ptr || !perm || sweeps < 0 || sweeps > 64 || (reverse != 0 && reverse != 1) ||
      (nnz > 0 && (!col_idx || !val)))
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
  if (edges_out) *edges_out = (int64_t)edges.size();
  std::vector<int32_t> deg((size_t)rows, 0);
  for (const auto &e : edges) { deg[e.first]++; deg[e.second]++; }
  std::vector<int64_t> start((size_t)rows + 1, 0);
  for (int64_t v = 0; v < rows; v++) start[v + 1] = start[v] + deg[v];
  std::vector<int32_t> nb(2 * edges.size());
  {
    std::vector<int64_t> at(start.begin(), start.end() - 1);
    for (const auto &e : edges) { nb[at[e.first]++] = e.second; nb[at[e.second]++] = e.first; }
  }
  const auto smaller = [&](int32_t a, int32_t b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; };
  for (int64_t v = 0; v < rows; v++) std::sort(nb.begin() + start[v], nb.begin() + start[v + 1], smaller);
  std::vector<int32_t> walk((size_t)rows);
  for (int64_t v = 0; v < rows; v++) walk[v] = (int32_t)v;
  std::sort(walk.begin(), walk.end(), smaller);

  std::vector<int32_t> pos((size_t)rows, -1), level((size_t)rows, -1), order((size_t)rows), queue, dist((size_t)rows, 0);
  std::vector<int64_t> seen((size_t)rows, -1);
  int64_t searches = 0, steps = 0;
  // the records of a search whose vertices stand in q[first, last) in search order with their levels in lv: one step
  // per level, its width and the sum of its list lengths
  const auto record = [&](int32_t k, const std::vector<int32_t> &q, int64_t first, int64_t last, const std::vector<int32_t> &lv) {
    for (int64_t h = first; h < last;) {
      int64_t width = 0, sum = 0;
      const int32_t l = lv[q[h]];
      for (; h < last && lv[q[h]] == l; h++) { width++; sum += deg[q[h]]; }
      if (steps < steps_cap) {
        if (kind) kind[steps] = k;
        if (size) size[steps] = width;
        if (looked) looked[steps] = sum;
      }
      steps++;
    }
  };
  // a breadth-first search from src -> its eccentricity; *last = the smallest vertex of its last level
  const auto search = [&](int32_t src, int32_t *last) {
    const int64_t gen = searches++;
    queue.clear();
    queue.push_back(src);
    seen[src] = gen; dist[src] = 0;
    for (size_t h = 0; h < queue.size(); h++) {
      const int32_t u = queue[h];
      for (int64_t j = start[u]; j < start[u + 1]; j++) {
        const int32_t w = nb[j];
        if (seen[w] == gen) continue;
        seen[w] = gen; dist[w] = dist[u] + 1;
        queue.push_back(w);
      }
    }
    record(0, queue, 0, (int64_t)queue.size(), dist);
    const int32_t ecc = dist[queue.back()];
    int32_t best = queue.back();
    for (size_t h = queue.size(); h-- > 0 && dist[queue[h]] == ecc;)
      if (smaller(queue[h], best)) best = queue[h];
    *last = best;
    return ecc;
  };
  int64_t done = 0;
  int32_t components = 0;
  for (int64_t t = 0; t < rows; t++) {
    const int32_t v = walk[t];
    if (pos[v] >= 0) continue;
    int32_t r = v;
    if (sweeps > 0 && deg[v] > 0) {
      int32_t x = v;
      int32_t e = search(r, &x);
      for (int32_t k = 0; k < sweeps && x != r; k++) {
        int32_t x2 = x;
        const int32_t e2 = search(x, &x2);
        if (e2 <= e) break;
        r = x; e = e2; x = x2;
      }
    }
    components++;
    const int64_t first = done;
    order[done] = r; pos[r] = (int32_t)done; level[r] = 0; done++;
    for (int64_t h = first; h < done; h++) {
      const int32_t u = order[h];
      for (int64_t j = start[u]; j < start[u + 1]; j++) {
        const int32_t w = nb[j];
        if (pos[w] >= 0) continue;
        order[done] = w; pos[w] = (int32_t)done; level[w] = level[u] + 1; done++;
      }
    }
    if (deg[r] > 0) record(1, order, first, done, level);   // (a vertex without an edge takes no step)
  }
  if (reverse)
    for (int64_t v = 0; v < rows; v++) pos[v] = (int32_t)(rows - 1 - pos[v]);
  for (int64_t v = 0; v < rows; v++) perm[pos[v]] = (int32_t)v;
  if (pos_out) std::copy(pos.begin(), pos.end(), pos_out);
  if (level_out) std::copy(level.begin(), level.end(), level_out);
  // bandwidth and profile under the identity ([0]) and the new order ([1])
  int64_t bw[2] = {0, 0}, prof[2] = {0, 0};
  for (int64_t v = 0; v < rows; v++) {
    int64_t lo[2] = {v, pos[v]};
    for (int64_t j = start[v]; j < start[v + 1]; j++) {
      const int64_t u = nb[j];
      lo[0] = std::min(lo[0], u); lo[1] = std::min<int64_t>(lo[1], pos[u]);
      bw[0] = std::max<int64_t>(bw[0], std::llabs(v - u)); bw[1] = std::max<int64_t>(bw[1], std::llabs((int64_t)pos[v] - pos[u]));
    }
    prof[0] += v - lo[0]; prof[1] += pos[v] - lo[1];
  }
  if (bandwidth) { bandwidth[0] = bw[0]; bandwidth[1] = bw[1]; }
  if (profile) { profile[0] = prof[0]; profile[1] = prof[1]; }
  if (components_out) *components_out = components;
  if (sweeps_out) *sweeps_out = (int32_t)searches;
  if (steps_out) *steps_out = steps;
  return 0;
}
