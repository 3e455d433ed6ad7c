/* sh_host.h -- C ABI of the host-side helpers (no HIP): synthetic matrix
 * generators and the MatrixMarket -> CSR loader used by the apps, the Python
 * binding and bench.py.  Built into sparseharness_amd/libsparseharness_host.so. */
#ifndef SH_HOST_H_
#define SH_HOST_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Seeded generators.  Caller allocates row_ptr[rows+1],
 * col_idx[nnz], val[nnz].  Return 0, -1 bad argument, -2 int32 overflow. */
int sh_synth_powerlaw(int64_t rows, int64_t cols, int64_t nnz, double exponent, int64_t dmax,
                      uint64_t seed, int32_t *row_ptr, int32_t *col_idx, float *val);
int sh_synth_rmat(int scale, int edge_factor, double a, double b, double c, uint64_t seed,
                  int permute, int32_t *row_ptr, int32_t *col_idx, float *val);

/* The strongly connected components of a square CSR pattern (Tarjan, single-threaded, iterative): the gold for sh_scc.
 * Entry (r, c) is the edge c -> r when 0 <= c < rows and its 32 value bits are not all zero; label[v] (rows words) becomes
 * the largest vertex index of v's component.  Return 0, -1 bad argument. */
int sh_scc_labels(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                  int32_t *label);

/* The weakly connected components of a square CSR pattern (union-find, single-threaded): the gold for sh_wcc.  Entry
 * (r, c) joins r and c when 0 <= c < rows and its 32 value bits are not all zero; label[v] (rows words) becomes the
 * largest vertex index of v's component.  Return 0, -1 bad argument. */
int sh_wcc_labels(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                  int32_t *label);

/* Exact triangle counts of the simple undirected graph under a square CSR pattern (clean, degree-orient, sort,
 * merge-intersect; single-threaded): the gold for sh_tri.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32
 * value bits are not all zero, in either direction, once.  tri[v] (rows 64-bit words) becomes the number of triangles
 * through v, deg[v] (rows words) its degree.  Return 0, -1 bad argument. */
int sh_triangle_counts(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                       uint64_t *tri, int32_t *deg);

/* The core numbers of the simple undirected graph under a square CSR pattern (clean, then the bucket algorithm of
 * Batagelj and Zaversnik; single-threaded, O(rows + edges) after the clean-up's sort): the gold for sh_core.  Entry (r, c)
 * counts when 0 <= c < rows, c != r and its 32 value bits are not all zero, in either direction, once.  core[v] (rows
 * words) becomes the largest k such that v lies in a subgraph whose vertices all have at least k neighbours in it, deg[v]
 * (rows words) its degree, *edges (may be NULL) the number of edges.  Return 0, -1 bad argument. */
int sh_core_numbers(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                    int32_t *core, int32_t *deg, int64_t *edges);

/* The support and the truss number of every edge of the simple undirected graph under a square CSR pattern (clean,
 * count the triangles through every edge, then the bucket algorithm of Wang and Cheng; single-threaded): the gold for
 * sh_truss.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not all zero, in either direction,
 * once.  Edge e of the *edges = M is the e-th smallest pair (u, v) with u < v: edge_u[e], edge_v[e]; support[e] the
 * triangles through it; truss[e] the largest k such that e lies in a subgraph all of whose edges are in at least k - 2
 * triangles of it (2 for an edge in no triangle).  The four arrays hold M <= nnz words each.  Return 0, -1 bad argument. */
int sh_truss_numbers(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                     int32_t *edge_u, int32_t *edge_v, int32_t *support, int32_t *truss, int64_t *edges);

/* The first-fit colouring of the simple undirected graph under a square CSR pattern in a fixed priority order (clean,
 * sort the vertices by their keys, one serial loop in that order; single-threaded): the gold for sh_color.  Entry (r, c)
 * counts when 0 <= c < rows, c != r and its 32 value bits are not all zero, in either direction, once.  v precedes u when
 * (primary(v), tie(v)) > (primary(u), tie(u)): primary = prio[v] when prio is not NULL, else the degree for order 2, else
 * 0; tie = the smaller index first for order 0, the larger mix32(v ^ seed) first for orders 1 and 2 (sh_color's mix32).
 * color[v] (rows words) becomes the smallest colour >= 0 that no preceding neighbour holds, depth[v] (rows words) the
 * length of the longest chain of preceding neighbours that ends in v, counted from 0 (the round in which sh_color
 * colours v), *colors (may be NULL) the largest colour plus 1, *edges (may be NULL) the number of edges.  Return 0, -1 bad
 * argument (order outside 0..2 included). */
int sh_greedy_colors(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                     int32_t order, uint32_t seed, const int32_t *prio, int32_t *color, int32_t *depth, int32_t *colors,
                     int64_t *edges);

/* The minimum spanning forest of the simple undirected graph under a square CSR matrix, its float32 values as weights
 * (clean, sort the keys, Kruskal's loop with a union-find; single-threaded): the gold for sh_msf.  Entry (r, c) counts
 * when 0 <= c < rows, c != r and its 32 value bits are not all zero.  Edge e is the e-th smallest pair u < v.  Weights are
 * compared by k(b) = b ^ 0xFFFFFFFF if the sign bit of the bits b is set, else b ^ 0x80000000; the weight of an edge is the
 * smallest, by k, over all counting entries (u, v) and (v, u); KEY(e) = k(weight[e]) << 32 | e, and the forest is what
 * Kruskal's algorithm returns when it takes the edges in ascending KEY.  edge_u, edge_v, weight (the 32 bits of the chosen
 * entry) and in_msf (1 or 0) hold nnz words each, of which *edges are written; comp[v] (rows words) becomes the largest
 * index of v's component; *components (may be NULL) the number of components.  Return 0, -1 bad argument. */
int sh_msf_edges(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                 int32_t *edge_u, int32_t *edge_v, uint32_t *weight, int32_t *in_msf, int32_t *comp, int64_t *edges,
                 int64_t *components);

/* The greedy weighted matching of the simple undirected graph under a square CSR matrix, its float32 values as weights
 * (clean, sort the edges by MKEY, take them in that order and keep an edge when both its ends are still free;
 * single-threaded): the gold for sh_match.  The edge rule, the edges and their weights are sh_msf_edges'.  MKEY(e) =
 * hi << 32 | lo with hi = k(weight[e]) for heavy == 0 (lightest first) and ~k(weight[e]) for heavy == 1 (heaviest first),
 * lo = e for seed == 0 and mix32(e ^ seed) otherwise (sh_color's mix32).  edge_u, edge_v, weight and in_match (1 or 0)
 * hold nnz words each, of which *edges are written; mate[v] (rows words) becomes the partner of v or -1; *pairs (may be
 * NULL) the number of matched edges.  Return 0, -1 bad argument (heavy outside {0, 1} included). */
int sh_greedy_matching(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                       int32_t heavy, uint32_t seed, int32_t *edge_u, int32_t *edge_v, uint32_t *weight, int32_t *in_match,
                       int32_t *mate, int64_t *edges, int64_t *pairs);

/* The reverse Cuthill-McKee ordering of the simple undirected graph under a square CSR pattern (clean, sort every list by
 * (deg, index), walk the vertices in ascending (deg, index), pick each component's root by George and Liu's searches with
 * a cap of `sweeps` beyond the first, number it from the root with one queue; single-threaded): the gold for sh_rcm, and
 * its definition.  Entry (r, c) counts when 0 <= c < rows, c != r and its 32 value bits are not all zero, in either
 * direction, once.  sweeps in [0, 64] (0: the first vertex of the walk is the root); reverse in {0, 1} (1: position k
 * becomes rows - 1 - k).  perm[k] (rows words) becomes the vertex at new position k; pos[v] and level[v] (rows words each;
 * may be NULL) its inverse and the level of v from its component's root; bandwidth[0], [1] and profile[0], [1] (may be
 * NULL) max |p(u) - p(v)| over the edges and the sum of p(v) - min(p(v), min over the neighbours) under the identity and
 * under the new order; *components, *searches (the searches run to find roots) and *edges may be NULL.  A step is one
 * level of one search, a search from a vertex with an edge only: kind[s] (0 a root search, 1 the numbering), size[s] (the
 * level's width) and looked[s] (the sum of its list lengths) are written for s < steps_cap (each may be NULL), *steps (may
 * be NULL) becomes the number of steps.  Return 0, -1 bad argument. */
int sh_rcm_order(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                 int32_t sweeps, int32_t reverse, int32_t *perm, int32_t *pos, int32_t *level, int64_t *bandwidth,
                 int64_t *profile, int32_t *components, int32_t *searches, int64_t *edges, int64_t steps_cap, int32_t *kind,
                 int64_t *size, int64_t *looked, int64_t *steps);

/* Betweenness centrality of the simple directed graph under a square CSR pattern (clean, then Brandes' two sweeps per
 * source with one queue; single-threaded): the gold for sh_bc.  Entry (r, c) is the edge c -> r when 0 <= c < rows, c != r
 * and its 32 value bits are not all zero; parallel entries are one edge.  Every sum is float64 in the order that
 * include/sparseharness_hip.h fixes (SUM), so the results equal sh_bc's bit for bit.  sources[n_sources] are taken in the
 * order given; accumulate in {0, 1} (1: the scores are added to what bc holds).  bc[v] (rows doubles); sigma[v] (rows
 * doubles) and level[v] (rows words) of the last source (each may be NULL); per source (each may be NULL): depth (the last
 * level that holds a vertex), reached (the source included), sigma_max and edges (the out-list entries walked forward).
 * Return 0, -1 bad argument. */
int sh_bc_scores(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                 const int32_t *sources, int32_t n_sources, int32_t accumulate, double *bc, double *sigma, int32_t *level,
                 int32_t *depth, int64_t *reached, double *sigma_max, int64_t *edges);

/* The sparse triangular solve T x = b of a square CSR matrix by plain substitution (single-threaded): the gold for
 * sh_trsv.  uplo 0 lower / 1 upper, unit 0 / 1 (the diagonal is one and stored diagonal entries are ignored).  Every
 * stored entry with 0 <= c < rows takes part whatever its value; entries of the other triangle and columns out of range
 * are ignored; rows need not be sorted and parallel entries are separate terms, in ascending (column, position as
 * given).  Every sum is float64 in the order that include/sparseharness_hip.h fixes (SUM of signed terms), so x equals
 * sh_trsv's bit for bit.  f32 0: b and x are rows doubles; 1: rows floats, b widened, x rounded once on the way out (later
 * rows read the unrounded value).  b and x may be the same array.  level[r] (rows words, may be NULL) = 0 for an empty
 * list, else 1 + the largest level in the list.  figures (6 words, may be NULL): list entries, levels, the longest list,
 * the widest level, the rows with d == 0 (0 when unit), the smallest such row or -1.  Return 0, -1 bad argument. */
int sh_trsv_solve(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val, const void *b,
                  int32_t uplo, int32_t unit, int32_t f32, void *x, int32_t *level, int64_t *figures);
/* SUM of n signed float64 terms as sh_trsv defines it.  tier 0: as sh_trsv chooses (one lane up to 8 terms, pieces
 * beyond); 1: the one-lane formula where n <= 8; 2: the pieces for any n.  The tiers are one function. */
double sh_trsv_list_sum(const double *t, int64_t n, int32_t tier);

/* The incomplete LU factorisation without fill, ILU(0), of a square CSR matrix by the row-wise IKJ recurrence
 * (single-threaded): the gold for sh_ilu0.  The slots of row r are the distinct columns 0 <= c < rows among its entries;
 * a[r, c] = its entries in the order given, widened to float64 and added left to right from +0.0; rows need not be
 * sorted and columns out of range take no part.  Every product and every subtraction is rounded once, in the order that
 * include/sparseharness_hip.h fixes, so lu equals sh_ilu0's bit for bit.  lu is in the positions of the entries: the
 * slot's value at the first entry of its (r, c) group, +0.0 at every other position; f32 1: nnz floats, rounded once on
 * the way out; 0: nnz doubles.  val and lu may be the same array when f32.  level[r] (rows words, may be NULL) = 0 for a
 * row without a lower slot, else 1 + the largest level among its lower slots.  figures (9 words, may be NULL): slots,
 * levels, the longest row in slots, the widest level, the rows without a diagonal slot, the smallest such row or -1, the
 * look-ups (work), the rows whose pivot == 0.0, the smallest such row or -1.  Return 0, -1 bad argument. */
int sh_ilu0_factor(int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val, int32_t f32, void *lu,
                   int32_t *level, int64_t *figures);

/* MatrixMarket -> CSR with the reference's semantics (SparseMatrix<T>,
 * src/sparse_matrix.cpp:11-119): see host/inc/sparse_matrix.h.  elem_is_int
 * selects SparseMatrix<int> (BFS) instead of SparseMatrix<float>.
 * truncate_values = 1 reproduces the reference's int narrowing (quirk A-3).
 * Returns 0 or the exit code the reference would have used (negative). */
typedef struct sh_host_csr {
  int32_t rows, cols, header_nnz;
  int64_t nnz;
  int32_t *row_ptr;
  int32_t *col_idx;
  void *val; /* float[nnz] or int32[nnz] */
} sh_host_csr;
int sh_mm_load(const char *path, int elem_is_int, int truncate_values, sh_host_csr *out);
/* As sh_mm_load, then the app's matrix normaliser before the narrowing: normalise = 0 none,
 * 1 SparseMatrix::pagerank_normalise(damping, 0) (app/pr.cpp:199), 2 scc_normalise()
 * (app/scc.cpp:217). */
int sh_mm_load_ex(const char *path, int elem_is_int, int truncate_values, int normalise, double damping,
                  sh_host_csr *out);
void sh_host_csr_release(sh_host_csr *m);

#ifdef __cplusplus
}
#endif
#endif
