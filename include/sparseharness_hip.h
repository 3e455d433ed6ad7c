/* sparseharness_hip.h -- C ABI of the MI355X-native CSR SpMV engine.
 *
 * This is the drop-in boundary for sparseharness's hot path.  The reference
 * has no FFI: its apps subclass Harness<TimingType,SemiRingType>
 * (inc/harness.h:11) and the "operator" is an OpenCL source string bound
 * positionally.  The entry points below are what that class's protected
 * helpers bind to once OpenCL is replaced by HIP; each one names the
 * reference interface it replaces (paths relative to the reference root).
 * The source-compatible C++ mirror that calls them lives in
 * sparseharness_amd/host/inc/harness.h; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every call returns int: SH_OK (0) or a negative SH_E* code; nothing
 *     exits the process (the reference's checkCLError -> exit(1),
 *     inc/opencl_utils.h:15-23, is re-created by the C++ mirror on top);
 *   - sh_last_error() gives the message of the last failing call on an engine
 *     (or of the last failing sh_engine_create when passed NULL);
 *   - the caller owns host memory, the engine owns device memory until the
 *     matching *_free / sh_engine_destroy;
 *   - one engine per host thread; an engine owns (or borrows) ONE hipStream_t
 *     and all its work is ordered on it (the reference has one in-order
 *     queue, inc/harness.h:79-80);
 *   - all vector/matrix elements are 4 bytes: float for SH_PLUS_TIMES_F32 and
 *     SH_MIN_PLUS_F32, int32 for SH_OR_AND_I32 and SH_MAX_MIN_I32;
 *   - there is NO CPU fallback: without a HIP device sh_engine_create fails
 *     with SH_ENODEVICE.
 */
#ifndef SPARSEHARNESS_HIP_H_
#define SPARSEHARNESS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SH_ABI_VERSION 3   /* 2: sh_plan_options lost the fused-launch fields and gained `fold`; sh_csr_footprint, sh_plan_row_work;
                              3: sh_row_pieces gained `gate`; sh_csr_piece_state */

enum {
  SH_OK = 0,
  SH_EINVAL = -1,    /* bad argument (null pointer, negative size, bad enum) */
  SH_ENODEVICE = -2, /* no usable HIP device / ordinal out of range */
  SH_EHIP = -3,      /* a HIP runtime call failed; see sh_last_error */
  SH_ENOMEM = -4,    /* host or device allocation failed */
  SH_ESHAPE = -5     /* operand sizes do not match the matrix */
};

/* Semirings = the user functions of example/{spmv,sssp,bfs}/kernel5.json:3
 *   PLUS_TIMES: mult l*r, add x+y, identity 0,       out = dot*alpha + y*beta
 *   MIN_PLUS:   mult |a|+|b|, add min(|a|,|b|), identity FLT_MAX,
 *               out = min(|dot|+|alpha|, |y|+|beta|)
 *   OR_AND:     mult (a!=0)&&(b!=0), add ||, identity 0,
 *               out = (dot&&alpha) || (y&&beta)
 *   MAX_MIN:    (example/scc/kernel5.json:3) mult min, add max, identity INT_MIN,
 *               out = max(min(dot,alpha), min(y,beta))
 * PageRank (example/pr/kernel5.json:3) is PLUS_TIMES with beta = (1-d)/N.      */
typedef enum {
  SH_PLUS_TIMES_F32 = 0,
  SH_MIN_PLUS_F32 = 1,
  SH_OR_AND_I32 = 2,
  SH_MAX_MIN_I32 = 3
} sh_semiring;

/* Launch geometry handed down from the run-file: replaces class Run
 * (inc/run.h:9-32) as consumed by Harness::executeKernel
 * (inc/harness.h:153-158).  The native kernels derive grid AND workgroup size
 * from the matrix schedule built at upload; the run's numbers are recorded by
 * the caller (they appear in the SQL row) and do not shape the launch.
 * May be NULL. */
typedef struct sh_launch {
  uint64_t global[3];
  uint64_t local[3];
} sh_launch;

typedef struct sh_engine sh_engine;
typedef struct sh_csr sh_csr;
typedef struct sh_vec sh_vec;

/* ---- engine: replaces Harness::Harness (inc/harness.h:13-82) ------------ */
int sh_abi_version(void);
/* Number of HIP devices (0 when none / no driver).  Never fails. */
int sh_device_count(void);
/* Create an engine on HIP device `device_ordinal` with its own stream. */
int sh_engine_create(int device_ordinal, sh_engine **out);
/* Same, but all work is enqueued on the caller's hipStream_t (e.g. the
 * current PyTorch stream) instead of an engine-owned one. */
int sh_engine_create_on_stream(int device_ordinal, void *hip_stream, sh_engine **out);
int sh_engine_destroy(sh_engine *e);
/* Replaces Harness::getDeviceName (inc/harness.h:100-107). */
int sh_engine_device_name(sh_engine *e, char *buf, size_t buflen);
/* Replaces deviceGetMaxAllocSize (inc/opencl_utils.h:216-226): free device bytes. */
int sh_engine_max_alloc(sh_engine *e, uint64_t *bytes);
/* Block until everything enqueued on the engine's stream has finished
 * (the reference waits after every enqueue, inc/harness.h:159). */
int sh_engine_synchronize(sh_engine *e);
const char *sh_last_error(const sh_engine *e);

/* ---- matrix: replaces SparseMatrix::cl_encode (src/sparse_matrix.cpp:122-399)
 *      + the two createAndUploadGlobalArg calls of Harness::allocateBuffers
 *      (inc/harness.h:201-205).  Takes the CSR view of the reference's row
 *      structure (row r = ellpackMatrix[r], stored order kept).  `val` is
 *      float[nnz] or int32[nnz] bit patterns.  Builds the device-side launch
 *      schedule (row blocks, long-row segments).  col_idx entries outside
 *      [0, cols) are legal and read as the semiring identity
 *      (bounds ladder of kernel5.json:3). */
int sh_csr_upload(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz,
                  const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                  sh_csr **out);
/* The same with explicit plan options instead of the environment.  sh_csr_upload
 * is sh_csr_upload_ex with sh_plan_options_from_env(): the SH_* variables are
 * read once per upload, never at launch time.  Zero-initialise, then call
 * sh_plan_options_default() and change what you need. */
typedef struct sh_plan_options {
  int32_t plan;            /* 0 auto (size rule, then timing when the columns are local), 1 stream, 2 tiled   [SH_PLAN]     */
  int32_t autotune;        /* 1: time both plans at upload when the rule says tiled and the columns are local [SH_AUTOTUNE] */
  int32_t value_coding;    /* 0 auto (4-bit / 8-bit dictionary codes when the data allows), 8: one-byte codes at most,
                              -1 off (raw 4-byte values)                                                      [SH_VALCODE]  */
  int32_t build_threads;   /* host threads of the layout build, 0 = min(hardware, 16)                         [SH_BUILD_THREADS] */
  int32_t heavy_per_tile;  /* rows averaging >= this many entries per column tile are pre-reduced in phase 1  [SH_HEAVY_PER_TILE] */
  int32_t chunk;           /* entries per phase-1 work item, 0 = by the number of items per CU (48 K or 64 K)  [SH_CHUNK]    */
  int32_t xcd_order;       /* 1: phase-1 work items ordered so that an XCD stages only its eighth of x        [SH_XCD_ORDER] */
  int32_t fold;            /* 1: phase 1 folds the entries of one row inside one column tile into ONE product before
                              it travels through P (a fifth of the light products of a power-law matrix)       [SH_FOLD]     */
  int32_t or_and_bits;     /* 1: also build the bit-blocked layout that SH_OR_AND_I32 launches then run on (x as a bitmap,
                              4 B per entry, no product array: a BFS iteration moves a third of the bytes); 2: ONLY
                              that layout (the matrix then serves SH_OR_AND_I32 alone)                          [SH_OR_AND_BITS] */
  int32_t build;           /* where the tiled layout is built: 0 default, 1 on the host (threads above), 2 on the device from
                              the CSR arrays (sorts and scans; a failed device step falls back to the host builder).
                              Both produce the same arrays, byte for byte                                    [SH_BUILD=host|device] */
  int32_t placement_tries; /* where hipMalloc puts the big arrays moves the time of one and the same layout by +-2 %: the
                              upload times this many placements of them and keeps the fastest (about 3 ms each for
                              a 200 M-entry matrix). 0 default (6 for matrices with >= 2^22 products, else 1), 1 = take the first         [SH_PLACEMENT_TRIES] */
} sh_plan_options;
void sh_plan_options_default(sh_plan_options *o);
void sh_plan_options_from_env(sh_plan_options *o);
/* Prefix sum (rows + 1 values, work_prefix[0] = 0) of the HBM bytes the engine expects to move per row under the
 * plan it would choose for a matrix of `cols` columns and `nnz` entries -- nnz is the size the PLAN is chosen for
 * (what one rank uploads, i.e. its share of the matrix), not necessarily row_ptr[rows]: what row-range sharding
 * across GPUs balances on (the reference has one device, inc/harness.h:419).  The weights describe the x-tiled and
 * the CSR-stream plan; they say nothing about the bit-blocked (or,and) layout (4 B per live entry: balance on the
 * entries).  Host-only: needs no device.  opt == NULL: the defaults. */
int sh_plan_row_work(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const sh_plan_options *opt,
                     uint64_t *work_prefix);
/* sh_csr_upload with the plan options given instead of read from the environment (opt == NULL: the defaults).  A forced
 * plan = 2 that the tiled layout's limits rule out (more than 65535 column tiles, more than 2^30 - 4 products, padding
 * above 25 %, ...: DESIGN.md 3, "Limits of the tiled layout") is not an error: the matrix runs on the CSR-stream plan,
 * and sh_csr_plan tells. */
int sh_csr_upload_ex(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz,
                     const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                     const sh_plan_options *opt, sh_csr **out);
int sh_csr_free(sh_engine *e, sh_csr *m);
/* Who built the matrix's tiled layout: *where = 0 host, 1 device; note (optional, cap bytes) = why the device builder
 * was not used although asked for, or empty. */
int sh_csr_builder(const sh_csr *m, int32_t *where, char *note, int64_t cap);
/* Placement trials of the upload (sh_plan_options::placement_tries): how many placements of the big arrays were timed,
 * the (+,x) launch time of the first one and of the one kept, in ms (0 when only one was tried). */
int sh_csr_placement(const sh_csr *m, int32_t *tries, float *first_ms, float *kept_ms);
int sh_csr_dims(const sh_csr *m, int64_t *rows, int64_t *cols, int64_t *nnz);
/* Algorithmic bytes of one SpMV over this matrix:
 * 8*nnz + 4*(rows+1) + 4*cols + 4*rows [+ 4*rows if y is read]. */
int sh_csr_algorithmic_bytes(const sh_csr *m, int reads_y, uint64_t *bytes);
/* Which execution plan sh_csr_upload chose (SH_PLAN=stream|tiled|auto overrides):
 * 0 = CSR-stream (x gathered from global memory, for L2-resident x),
 * 1 = x-tiled two-phase (x tiles staged in LDS, products re-binned through HBM),
 * 2 = the bit-blocked (or,and) layout alone (sh_plan_options::or_and_bits = 2).
 * streamed_bytes = HBM bytes one SpMV moves by construction under that plan (tiled: 2.5, 3 or 6 B per
 * stream entry + 4 B written and ~6.2 B re-read per product that travels through P + the vectors; the
 * measured figure of a layout is in profiles/measured_traffic.json). */
int sh_csr_plan(const sh_csr *m, int32_t *plan, uint64_t *streamed_bytes);
/* One-line description of the layout built at upload, for logs and bench records, e.g.
 * "tiled values=dict4(16) tiles=306 chunks=3420 bins=6750 heavy_rows=5276 stream=216M light=133.9M products=109M folded"
 * (stream: entries phase 1 reads, padding included; light: entries of light rows; products: what travels through P).
 * values=dict8(k) / dict4(k): the matrix has k <= 256 / <= 16 distinct 4-byte values and the tiled stream
 * carries one-byte / four-bit codes (lossless; SH_VALCODE=8 stops at one-byte codes, SH_VALCODE=off keeps
 * raw values); values=raw otherwise.
 * " tuned(stream=..ms,tiled=..ms)" is appended when the plan was confirmed by timing both at upload:
 * large matrices get the tiled plan by size; when their columns are local (row bins touch less than
 * half of the column tiles) both plans are timed and the CSR-stream plan is kept if > 10 % faster; SH_PLAN=stream|tiled or SH_AUTOTUNE=0 skip the timing. */
int sh_csr_describe(const sh_csr *m, char *buf, size_t buflen);
/* Device memory the matrix holds (the arrays of the plan that runs; the CSR arrays themselves -- 8 B per entry --
 * are uploaded only for the CSR-stream plan or while both plans are timed at upload).  The reference keeps its
 * padded ELLPACK buffers for the life of the process (inc/harness.h:197-250, never released). */
int sh_csr_footprint(const sh_csr *m, uint64_t *device_bytes);

/* ---- vectors: replace createAndUploadGlobalArg / createGlobalArg /
 *      writeToGlobalArg / fillGlobalArg / readFromGlobalArg
 *      (inc/harness.h:266-391) for x, y, output ------------------------- */
int sh_vec_alloc(sh_engine *e, int64_t n, sh_vec **out);
/* Wrap device memory owned by someone else (e.g. a torch tensor); never freed
 * by the engine. */
int sh_vec_wrap(sh_engine *e, void *device_ptr, int64_t n, sh_vec **out);
int sh_vec_free(sh_engine *e, sh_vec *v);
int sh_vec_upload(sh_engine *e, sh_vec *v, const void *host, int64_t n);   /* blocking */
int sh_vec_download(sh_engine *e, const sh_vec *v, void *host, int64_t n); /* blocking */
int sh_vec_fill(sh_engine *e, sh_vec *v, uint32_t pattern32);              /* async   */
int sh_vec_copy(sh_engine *e, sh_vec *dst, const sh_vec *src);             /* async   */
int64_t sh_vec_len(const sh_vec *v);
void *sh_vec_device_ptr(const sh_vec *v);

/* ---- the hot path: replaces Harness::executeKernel (inc/harness.h:149-195)
 *      running a Lift kernel (example/<algo>/kernel*.json:3):
 *        out[r] = epilogue( (+)_j ( x[col_j] (x) val_j ), alpha, y[r], beta )
 *      alpha/beta point to one element of the semiring's type.  y may be NULL
 *      when the epilogue does not read it (PLUS_TIMES or OR_AND with beta==0,
 *      MAX_MIN with beta==INT_MIN).
 *      out must not alias x.  If kernel_ns != NULL the call waits and returns
 *      the device time of the launch(es) in ns (hipEvent START->STOP, as the
 *      reference's CL_PROFILING_COMMAND_START/END, inc/harness.h:183-194);
 *      if NULL the call only enqueues. */
int sh_spmv(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x,
            const sh_vec *y, const void *alpha, const void *beta, sh_vec *out,
            const sh_launch *launch, uint64_t *kernel_ns);

/* ---- iterative apps: replaces the do/while of HarnessSSSP::executeRun +
 *      should_terminate_iteration (app/sssp.cpp:97-176) and the BFS twin
 *      (app/bfs.cpp:94-174) with an on-device loop: the convergence test is
 *      fused into the kernel epilogue (float: |in-out| < delta, int: ==) and
 *      only one flag word per iteration crosses PCIe.
 *        launch k: out = kernel(in, y); y aliases in after launch 0.
 *      x holds x0 on entry and the final vector on return (the buffer the
 *      reference's `input` pointer designates after its last swap); y0 is
 *      read by launch 0 only; scratch is clobbered.  *iters counts launches
 *      including the confirming one; max_iters bounds non-terminating graphs
 *      (TODO.md:7-8).  ns_per_iter (may be NULL, capacity max_iters) receives
 *      each launch's device time; total_ns their sum (MULTI_ITERATION_SUM,
 *      app/sssp.cpp:77-84). */
/* The same step for a matrix whose rows live in PIECES of the vectors (multi-GPU iteration driver: the vectors
 * interleave the pieces of all ranks so that piece c of every rank is one contiguous region to all-gather; the
 * reference has one device and no counterpart, app/sssp.cpp:112-153 is the loop this serves).  Row r belongs to
 * piece c = r / piece_rows and is element element_of_piece[c] + (r - c * piece_rows) of out, of y and -- for the
 * convergence test -- of x.  With report != 0 the launch tells when each piece is complete: *done_words then points
 * to n_pieces words in host memory (owned by the matrix) and word c reaches *round once every row of piece c is
 * written and visible system-wide, pieces completing in ascending order while the launch is still running, so the
 * caller can start exchanging piece c while later pieces are being computed.  ONE launch of the ordinary plan: no
 * per-piece matrices.  At most 8 pieces. */
typedef struct sh_row_pieces {
  int32_t n_pieces;
  int32_t piece_rows;
  int64_t element_of_piece[8];
  int32_t report;
  int32_t reserved;
  const int32_t *gate;   /* device word or NULL: a launch whose gate word is 0 when it starts returns at once and writes nothing
                            (what sh_iterate does internally: a caller that enqueues iteration k + 1 before it has read the
                            flags of iteration k passes the device-side OR of those flags here).
                            A gated launch cannot report: report != 0 together with a gate is refused with SH_EINVAL (a
                            launch that writes nothing has no piece to report, and a caller polling *done_words would
                            wait for a round that never comes).  A refused call leaves *round where it was. */
} sh_row_pieces;
int sh_spmv_step_pieces(sh_engine *e, sh_semiring sr, sh_csr *A, const sh_vec *x, const sh_vec *y,
                        const void *alpha, const void *beta, sh_vec *out, const sh_row_pieces *pieces, double delta,
                        int32_t *changed_flag_device, uint32_t *round, const volatile uint32_t **done_words);

/* Diagnosis for a caller whose wait on *done_words timed out (no counterpart in the reference): host_words[8] = the
 * words the caller polls, *round = the latest reporting launch, *expected = arrivals per piece it waits for,
 * arrivals[8] = the device-side arrival counters of that launch, read through a stream of the call's own so that a
 * launch that never ends cannot block the question (0xFFFFFFFF each when even that copy did not finish in 2 s). */
int sh_csr_piece_state(sh_engine *e, sh_csr *A, uint32_t *arrivals, uint32_t *host_words, uint32_t *expected, uint32_t *round);

int sh_iterate(sh_engine *e, sh_semiring sr, const sh_csr *A, sh_vec *x,
               const sh_vec *y0, sh_vec *scratch, const void *alpha,
               const void *beta, double delta, int32_t max_iters,
               const sh_launch *launch, int32_t *iters, int32_t *converged,
               uint64_t *ns_per_iter, uint64_t *total_ns);

/* One iteration step for callers that drive the loop themselves (the
 * multi-GPU driver): out = kernel(x, y) and *changed_flag (device int32,
 * may be NULL) is set to 1 if any row fails the convergence test against
 * `x`.  x/out may address a longer (replicated) vector: row r of this matrix
 * compares x[out_row_offset + r] with out[r].  Enqueue only. */
int sh_spmv_step(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x,
                 const sh_vec *y, const void *alpha, const void *beta, sh_vec *out,
                 int64_t x_row_offset, double delta, int32_t *changed_flag_device);

/* ---- several vectors per launch: extends Harness::executeKernel (inc/harness.h:149-195) and the do/while of
 *      HarnessSSSP::executeRun (app/sssp.cpp:97-176).  The reference multiplies by ONE vector per launch and runs
 *      `trials` repetitions of one source; it has no counterpart of the two calls below.
 *      The matrix stream (8 B per entry) is read once for `width` vectors, and the gather of a column fetches
 *      4 * width contiguous bytes instead of 4.  Measured on an MI355X (DESIGN.md "Multi-vector products",
 *      profiles/spmm_*.json), as t_spmm / (width * t_spmv under the default plan):
 *        - x * width cache-resident (170 998 rows, 0.96 M entries): 0.48 / 0.34 / 0.25 / 0.19 at width 4 / 8 / 16 / 32;
 *        - a matrix that sh_csr_upload gives the x-tiled plan (R-MAT-23: 8.4 M rows, 134 M entries, scattered columns):
 *          1.6 at width 4 -- NOT worth calling: four tiled sh_spmv are faster -- then 0.81 / 0.43 / 0.33 at 8 / 16 / 32.
 *          On the power-law 10 M-row / 200 M-entry matrix (uniform columns): 2.4 and 1.2 at width 4 and 8 -- NOT worth
 *          calling -- then 0.61 / 0.40 at 16 / 32.
 *          Against `width` launches on the same CSR-stream arrays it is 3.4 to 21 times faster at every width.
 *        Rule: call it when the matrix' default plan is the CSR-stream plan; otherwise only from width 16 on.
 *
 * K vectors per launch.  X, Y, Out are ordinary sh_vec of >= cols*width (X) / rows*width (Y, Out) elements,
 * element i of vector j at i*width + j, 16-byte aligned.  width in {4, 8, 16, 32}.  alpha, beta: one element, shared by
 * the columns.  Y may be NULL where sh_spmv allows it.
 * The matrix must hold its CSR arrays on the device (uploaded with sh_plan_options::plan = 1, or chosen so by the
 * size rule); otherwise SH_EINVAL with a message that says how to upload.  Out must not alias X.
 * One launch (plus the long-row fix-up when the matrix has rows above the schedule's threshold).  kernel_ns as sh_spmv.
 * NOT covered by the multi-vector path: the x-tiled and the bit-blocked plans, row pieces / `report`
 * (sh_spmv_step_pieces) and the multi-GPU driver. */
int sh_spmm(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, const sh_vec *X, const sh_vec *Y,
            const void *alpha, const void *beta, sh_vec *Out, uint64_t *kernel_ns);

/* sh_iterate for `width` independent start vectors at once (multi-source SSSP / BFS / SCC labels).
 * Column j stops at the first launch in which none of its rows fails the convergence test; from then on it is FROZEN:
 * later launches carry it through unchanged while the other columns go on.  On return column j of X is bit-identical
 * to what sh_iterate leaves in x when run on that column alone, iters_of_column[j] equals its *iters and
 * converged_of_column[j] its *converged.  *launches = max_j iters_of_column[j] (<= max_iters).
 * (For SH_PLUS_TIMES_F32 "alone" means through this path: a row's sum is taken in another order than under sh_spmv,
 * so the last bits, and with them a count that hangs on |in - out| < delta by a hair, may differ from sh_iterate's.)
 * X, Y0, scratch: rows*width elements each (the matrix must be square); scratch is clobbered and must not alias X.
 * iters_of_column, converged_of_column: `width` words; ns_per_launch (may be NULL): capacity max_iters.
 * max_iters <= 0: nothing is launched, *launches = 0.  The launches are enqueued ahead of the host as sh_iterate's are:
 * the per-column flags of launch i live in device memory and launch i + 1 reads them as its live columns; the loop ends
 * when every column is frozen.  Row pieces / `report` / multi-GPU are out of scope here as for sh_spmm. */
int sh_iterate_multi(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, sh_vec *X, const sh_vec *Y0,
                     sh_vec *scratch, const void *alpha, const void *beta, double delta, int32_t max_iters,
                     int32_t *launches, int32_t *iters_of_column, int32_t *converged_of_column,
                     uint64_t *ns_per_launch, uint64_t *total_ns);

/* ---- (or,and) on packed bits: extends Harness::executeKernel (inc/harness.h:149-195) and the BFS loop of
 *      HarnessBFS::executeRun (app/bfs.cpp:94-174).  The reference runs `trials` repetitions of ONE source, one int32
 *      per vertex; it has no counterpart of the four calls below.
 *      The (or,and) semiring only has the values 0 and 1, so a vertex carries `words` 32-bit words for 32 * words
 *      sources: word w of vertex v is element v*words + w of an ordinary sh_vec, source s is bit s % 32 of word s / 32.
 *      One launch reads the matrix stream once and gathers 4 * words contiguous bytes per entry -- the gathers and, at
 *      words = 1, the bytes of ONE sh_spmv -- for all 32 * words sources:
 *        Out[r*words + w] = ( OR over entries e of row r with val_e != 0 and 0 <= col_e < cols of X[col_e*words + w]  &  amask )
 *                         | ( Y[r*words + w] & bmask ),     amask = alpha != 0 ? ~0 : 0, bmask likewise from beta
 *      which is SH_OR_AND_I32's mul / add / epilogue on every bit on its own.
 *      Measured on an MI355X (DESIGN.md "Bit-parallel multi-source BFS", profiles/msbfs_*.json): as t_bits_iterate / (cost of the same
 *      32 * words sources another way), alpha = beta = 1 from random sources to convergence, at words = 1 / 2 / 4 / 8:
 *        - against 32 * words single-source sh_iterate runs under the matrix' default plan:
 *            x cache-resident (170 998 rows, 0.96 M entries, stream plan):        0.042 / 0.024 / 0.014 / 0.012
 *            R-MAT-23 (8.4 M rows, 134 M entries, x-tiled plan):                  0.25  / 0.29  / 0.13  / 0.060
 *            power-law 10 M rows / 200 M entries (x-tiled plan):                  0.26  / 0.14  / 0.074 / 0.041
 *        - against words x sh_iterate_multi at width 32 on the same CSR arrays:  0.20 / 0.11 / 0.065 / 0.055,
 *            0.42 / 0.23 / 0.14 / 0.074 and 0.58 / 0.31 / 0.16 / 0.090 on the same three matrices.
 *        A launch costs what one sh_spmv on the CSR arrays costs (R-MAT-23: 1.62 ms at words = 1, 2.26 ms at words = 8).
 *        Rule: with 32 or more (or,and) start vectors call it, on a plan = 1 upload, whatever the matrix' default plan,
 *        with the largest `words` the sources fill; every `words` pays on every matrix class measured.  With fewer than
 *        about 8 sources on a matrix whose default plan is x-tiled, single-source sh_iterate runs stay cheaper.
 *
 * words in {1, 2, 4, 8}.  alpha, beta: one int32 each, as for SH_OR_AND_I32 in sh_spmv, shared by all sources.
 * X >= cols*words, Y / Out >= rows*words elements, 16-byte aligned; Y may be NULL when beta == 0; Out must not alias X.
 * The matrix must hold its CSR arrays on the device (uploaded with sh_plan_options::plan = 1, or chosen so by the
 * size rule); otherwise SH_EINVAL with a message that says how to upload.  A matrix without rows launches nothing.
 * One launch (plus the long-row fix-up when the matrix has rows above the schedule's threshold).  kernel_ns as sh_spmv.
 * NOT covered by the packed path: the x-tiled and the bit-blocked plans, row pieces / `report` (sh_spmv_step_pieces),
 * the multi-GPU driver and the C++ harness apps. */
int sh_bits_spmv(sh_engine *e, const sh_csr *A, int32_t words, const sh_vec *X, const sh_vec *Y,
                 const void *alpha, const void *beta, sh_vec *Out, uint64_t *kernel_ns);

/* sh_iterate(SH_OR_AND_I32) for 32 * words start vectors at once (bit-parallel multi-source BFS).
 * Source s stops at the first launch that changes none of its bits; from then on it is FROZEN: later launches carry
 * its bits through while the other sources go on.  (Needed, not only an optimisation: launch 0 reads Y0 and later
 * launches the previous vector, so a source confirmed at launch 0 is not necessarily a fixed point of the later
 * launches; and with beta == 0 a source may oscillate and never converge.)  On return bit s of X equals, for every
 * vertex, (x != 0) of what sh_iterate(SH_OR_AND_I32) leaves when run alone on the 0/1 vector of source s with the same
 * alpha, beta, max_iters and bit s of Y0 as its y0; iters_of_source[s] equals its *iters, converged_of_source[s] its
 * *converged; *launches = max_s iters_of_source[s] (<= max_iters).
 * X, Y0, scratch: rows*words elements each (the matrix must be square); scratch is clobbered and must not alias X.
 * iters_of_source, converged_of_source: 32 * words entries; ns_per_launch (may be NULL): capacity max_iters.
 * newly_set (may be NULL): host memory of max_iters * 32*words words; entry l * 32*words + s receives the number of
 * vertices whose bit s was 0 before launch l and 1 after it (0 for a frozen source and for launches that did not
 * run).  With alpha = beta = 1 and Y0 = X this is the number of vertices at BFS distance l + 1 from source s:
 * eccentricity and closeness of 32 to 256 sources from one sweep, without unpacking a vector.
 * max_iters <= 0: nothing is launched, *launches = 0.  The launches are enqueued ahead of the host as sh_iterate_multi's
 * are: the changed words of launch i live in device memory and launch i + 1 reads them as its live mask; the loop
 * ends when every source is frozen. */
int sh_bits_iterate(sh_engine *e, const sh_csr *A, int32_t words, sh_vec *X, const sh_vec *Y0, sh_vec *scratch,
                    const void *alpha, const void *beta, int32_t max_iters, int32_t *launches,
                    int32_t *iters_of_source, int32_t *converged_of_source, uint32_t *newly_set,
                    uint64_t *ns_per_launch, uint64_t *total_ns);

/* Between the packed form and the 0/1 int32 vectors of sh_spmv, sh_iterate and the apps; source in [0, 32 * words).
 * sh_bits_from_column: bit `source` of B[i*words + source/32] := (v[i] != 0) for i < n, the other bits untouched.
 * sh_bits_to_column:   v[i] := that bit as int32 0 / 1.   v >= n, B >= n*words elements.
 * Both are asynchronous on the engine's stream. */
int sh_bits_from_column(sh_engine *e, const sh_vec *v, int64_t n, int32_t words, int32_t source, sh_vec *B);
int sh_bits_to_column(sh_engine *e, const sh_vec *B, int64_t n, int32_t words, int32_t source, sh_vec *v);

/* ---- frontier-driven iteration: extends the do/while of HarnessSSSP::executeRun (app/sssp.cpp:97-176), its BFS twin
 *      (app/bfs.cpp:94-174) and Harness::executeKernel (inc/harness.h:149-195).  The reference launches its kernel over
 *      the whole matrix every time; it has no counterpart of the calls below.
 *      sh_iterate's launches are dense: each reads the whole matrix, whatever the launch before changed.  From launch 1
 *      on a launch computes x_{k+1}[r] from x_k[r] and x_k[col_j] over row r's entries, so a row none of whose inputs
 *      changed between x_{k-1} and x_k keeps its word.  sh_iterate_frontier recomputes, from launch 2 on and while the
 *      wavefront is thin, only
 *        active_k = C_k  u  { r : row r has an entry with 0 <= col < cols and col in C_k },  C_k = rows whose bits changed,
 *      found through the pattern of the transposed matrix and recomputed by a row gather on the CSR arrays, in place.
 *      min / or / max are order-free, so every iterate, *iters and *converged equal sh_iterate's bit for bit, for any
 *      alpha, beta, x0, y0 (promised for vectors without NaN / infinity; (min,+) needs delta > 0: an untouched row must
 *      not fail |in - out| < delta).
 *      Measured on an MI355X (DESIGN.md "Frontier-driven iteration", profiles/frontier_*.json), total device time as a
 *      ratio to sh_iterate under the matrix' default plan, at dense_share = 0 (detection only) / the default / 1:
 *        - 2048 x 2048 grid graph, BFS (4095 launches):   1.52 / 0.43 / 0.44    SSSP, weights 1..16 (4198):  1.89 / 1.57 / 2.27
 *        - 170 998 rows, 0.96 M entries (23 / 27 launches of 17 us): 2.1 / 4.2 / 6.6 and 2.5 / 4.4 / 9.2
 *        - R-MAT-23 (8 / 10 launches of 0.29 ms):           1.27 / 3.1 / 15.7 and 1.31 / 3.3 / 18.5
 *        A sparse launch costs about 25 us at least (four small kernels); detection adds 30 to 90 us to a dense launch.
 *        Rule: call it for runs of hundreds of launches or more on a matrix with bounded row and column lengths (meshes,
 *        grids, road-like graphs) whose dense launch costs well above 30 us and in which a vertex changes a few times at
 *        most (BFS, reachability, label propagation).  For power-law graphs, runs of a few dozen launches and small
 *        matrices sh_iterate is faster; no dense_share serves both kinds, the default (0.02) is the grid's best.
 *
 * sh_frontier_create: A is square and was uploaded (under ANY plan) from the host arrays given here, which the call
 * reads again.  The handle holds on the device: row_ptr / col_idx / val (borrowed from A when A keeps its CSR arrays --
 * A must then outlive the handle -- copied otherwise), the pattern of the transpose (col_ptr[cols + 1], row_of[nnz];
 * entries with col outside [0, cols) are left out), two worklists, a stamp word and a value word per row, two lists of
 * pieces of long columns / rows.  The transpose is built on the device (column histogram, exclusive scan, scatter).
 * sh_frontier_footprint: device bytes held =
 *     (CSR arrays copied ? 4 * (rows + 1) + 8 * nnz : 0)  +  4 * (cols + 1) + 4 * nnz  +  16 * rows
 *     + 8 * (nnz / 1024 + 1) + 8 * (nnz / 2048 + 1) + 512.
 * sh_frontier_transpose (tests, tools): col_ptr receives cols + 1 words, row_of as many as col_ptr[cols]; either may be
 * NULL.  The order of the rows inside one column is unspecified.
 *
 * sh_iterate_frontier: sh_iterate's contract for x / y0 / scratch / alpha / beta / delta / max_iters / iters / converged /
 * ns_per_iter / total_ns, and the same result bit for bit.  Of x and scratch (vectors of >= rows elements) `rows` elements
 * are overwritten, no more; y0 is only read.  f may serve any number of calls, one at a time.
 * dense_share: a launch k >= 2 runs sparse when (entries of the transposed columns in C_k) <= dense_share * nnz, dense
 *   otherwise (launches 0 and 1 are always dense).  0: every launch dense (sh_iterate plus the change detection);
 *   >= 1: every launch from 2 on sparse; negative: the engine's default.
 * mode_per_iter / changed_per_iter / active_per_iter (each may be NULL, capacity max_iters): per launch that ran, 0 dense /
 *   1 sparse; |C| AFTER the launch (rows whose bits it changed); rows recomputed (= rows for a dense launch).
 * The launches are enqueued ahead of the host as sh_iterate's are, up to 8 of ONE mode; the device closes the gate of
 * the launches behind a change of mode (or the end of the loop), so the host joins in once per batch and per change.
 * Outside the contract: a word of SH_MIN_PLUS_F32 that is Inf or NaN and STAYS so (alpha = Inf, say; with alpha finite a
 *   launch replaces an Inf by a value <= FLT_MAX).  Its bits do not change, so it joins no changed list, while
 *   |Inf - Inf| is NaN and fails sh_iterate's `|in - out| < delta` at every launch: sh_iterate runs to max_iters
 *   unconverged; sh_iterate_frontier does the same while its launches are dense (dense_share = 0: always) and reports
 *   converged at its first sparse launch, whose active set is empty -- launch 2 at the earliest.  The vector is the
 *   same either way (tests/test_minplus_gpu.py pins both).
 * SH_EINVAL: SH_PLUS_TIMES_F32 (a recomputed row would have to reproduce the summation order of whichever plan ran the
 * dense launches), delta <= 0 with SH_MIN_PLUS_F32, max_iters < 1, a handle made for another matrix.
 * NOT covered: SH_PLUS_TIMES_F32, sh_iterate_multi / sh_bits_iterate, row pieces (sh_spmv_step_pieces), the multi-GPU
 * driver and the C++ harness apps. */
typedef struct sh_frontier sh_frontier;
int sh_frontier_create(sh_engine *e, const sh_csr *A, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                       const void *val, sh_frontier **out);
int sh_frontier_free(sh_engine *e, sh_frontier *f);
int sh_frontier_footprint(const sh_frontier *f, uint64_t *device_bytes);
int sh_frontier_transpose(sh_engine *e, const sh_frontier *f, int32_t *col_ptr, int32_t *row_of);
int sh_iterate_frontier(sh_engine *e, sh_semiring sr, const sh_csr *A, sh_frontier *f, sh_vec *x, const sh_vec *y0,
                        sh_vec *scratch, const void *alpha, const void *beta, double delta, int32_t max_iters,
                        double dense_share, int32_t *iters, int32_t *converged, int32_t *mode_per_iter,
                        int64_t *changed_per_iter, int64_t *active_per_iter, uint64_t *ns_per_iter, uint64_t *total_ns);

/* ---- direction-optimising BFS with levels and parents: extends the BFS loop of HarnessBFS::executeRun
 *      (app/bfs.cpp:94-174) and Harness::executeKernel (inc/harness.h:149-195).  The reference's BFS is an SpMV loop on
 *      the (or,and) semiring whose answer is a 0/1 reachability vector; it has no counterpart of the calls below.
 *      sh_bfs_levels is a BFS that is an algorithm of its own (Beamer, Asanovic, Patterson, SC 2012): it answers HOW FAR
 *      every vertex is from the sources and, on request, THROUGH WHICH vertex it was reached.  In thin levels it goes
 *      top-down over the out-edges of the frontier only; in fat levels bottom-up, where an unvisited row stops at its
 *      first entry whose column is in the frontier -- the early exit that the semiring contract forbids to sh_spmv.
 *
 *      An EDGE c -> r exists when row r stores an entry with column c, 0 <= c < rows, and a value whose 32 bits are not
 *      all zero: exactly the entries that can switch a row on under SH_OR_AND_I32.  The SOURCES are the v with x0[v] != 0.
 *        level[v]  = 0 for a source, else k + 1 where launch k (from 0) of sh_iterate(SH_OR_AND_I32, alpha = 1, beta = 1,
 *                    y0 = x0) is the first whose output has x[v] != 0; -1 if there is none (the BFS distance);
 *        parent[v] = -1 for sources and unreached vertices, else the SMALLEST c with an edge c -> v and
 *                    level[c] == level[v] - 1 (canonical: one extra row-parallel pass after the traversal, run only when
 *                    `parent` is given; the traversal itself carries no parent atomics);
 *        *depth = the largest level assigned, *reached = vertices with level >= 0, *complete = 1 when the frontier ran
 *                    empty, 0 when max_levels steps were used up first (levels above max_levels stay -1).
 *      Step L assigns level L + 1 from the vertices at level L; it runs while that frontier is not empty and
 *      L < max_levels.  A complete search runs depth + 1 steps (the last finds nothing, as sh_iterate's confirming
 *      launch), so sh_iterate's *iters == depth + 1; a search cut at max_levels == depth reports complete = 0.
 *      The result does not depend on the direction any step ran in.
 *
 *      Measured on an MI355X (DESIGN.md "6e Direction-optimising BFS", profiles/bfs_levels_*.json), total device time at
 *      the default shares as a ratio to sh_iterate(SH_OR_AND_I32) under the matrix' default plan / to sh_iterate_frontier at
 *      its default share, without the parent pass, from vertex 0 and two random sources:
 *        - R-MAT-23 (8.4 M rows, 134 M entries; 7-8 launches, 2.1-2.4 ms):   0.44-0.47 / 0.11-0.23; with parents 1.15-1.25
 *        - power-law 10 M rows / 200 M entries (11 launches, 4.4 ms):        0.58-0.62 / 0.19;      with parents 1.36-1.40
 *        - 2048 x 2048 grid graph (3087-4095 launches, 187-251 ms):          0.38-0.42 / 0.84-0.96; with parents the same
 *        - 170 998 rows, 0.96 M entries (22-23 launches of 17 us, 0.4 ms):   1.54-1.62 / 0.34-0.37; with parents 1.60-1.68
 *        The bottom-up steps looked at 5 to 24 % of the edges per step (R-MAT-23: 22 M of 134 M in its fattest level).  A step
 *        costs 16 to 25 us at least (four dependent launches, two of them empty: all of the grid's 24-26 us per level, and why
 *        the small matrix loses); a top-down step over a fat level is the expensive one (1.5 M edges: 0.9 ms), which is why
 *        Beamer's 1/14 loses on the power-law matrix (2.3) and the default turns bottom-up at 0.5 % of the edges.  The parent
 *        pass gathers level[] once per edge: 1.65 ms on R-MAT-23, 3.4 ms on the power-law matrix -- more than the search.
 *        Rule: call it when you need levels or parents.  For reachability alone call it (without `parent`) on matrices whose
 *        sh_iterate launch costs well above 25 us -- large power-law graphs and grids / meshes alike --; on small matrices
 *        (a launch of under 25 us) sh_iterate stays faster.  No pair of shares makes the small matrix win.
 *
 * sh_bfs_graph_create: the handle is made from the host CSR arrays alone (no sh_csr: the search runs on a layout of its
 * own, whatever plan the matrix was uploaded under).  The matrix is square (rows x rows); col_idx outside [0, rows) and
 * stored zeros are legal and are no edges.  The handle holds on the device: the edge pattern by rows (in_ptr[rows + 1],
 * in_col[edges], stored order of the survivors kept: 4 B per edge), its transpose (out_ptr[rows + 1], out_row[edges],
 * order inside one list unspecified), two vertex queues, two frontier bitmaps (one bit per vertex), two lists of pieces
 * of long out-lists, the pieces of long rows, a control block.  Built on the device (flag per entry, exclusive scan,
 * compaction; column histogram, scan, scatter).  rows == 0 gives a valid handle.
 * sh_bfs_graph_footprint: device bytes held, with W = (rows + 31) / 32 =
 *     8 * (rows + 1) + 8 * edges  +  8 * rows  +  8 * W  +  16 * (edges / 1024 + 1)  +  8 * (edges / 2048 + 1)  +  18432.
 * sh_bfs_graph_edges: the entries kept as edges.
 *
 * sh_bfs_levels: level, parent (may be NULL): int32 vectors of >= rows elements; `rows` elements of each are overwritten,
 * no more; x0 is only read (`rows` elements, no more); level and parent must not alias x0 or each other.  g may serve
 * any number of calls, one at a time.
 * max_levels >= 1.  The per-level arrays (each may be NULL) have capacity max_levels + 1 for size_per_level (entry 0 =
 * the number of sources, entry L + 1 = vertices step L assigned) and max_levels for the others; one entry per step that
 * ran, entries beyond are not written.
 * mode_per_level[L]: 0 = step L ran top-down, 1 = bottom-up.  edges_per_level[L]: edges the step looked at -- top-down:
 *   exactly the sum of the out-list lengths of its frontier; bottom-up: what the early exit left (informational: rows
 *   above 32 edges are searched 64 edges at a time, and a whole group counts).
 * ns_per_level / total_ns: device time (hipEvent) as elsewhere; total_ns also holds the set-up launch and the parent pass.
 * The switching rule, with E = edges, n = rows, F_L = the vertices at level L, m_L = the sum of their out-list lengths:
 *   step 0 is top-down unless m_0 > up_share * E; a step after a top-down step is bottom-up iff m_L > up_share * E; a
 *   step after a bottom-up step is top-down iff |F_L| < down_share * n; otherwise the direction stays (all in double
 *   arithmetic).  up_share >= 1: top-down throughout; up_share = down_share = 0: bottom-up throughout (unless m_0 = 0: sources without
 *   out-edges, whose only step then runs top-down over nothing); a negative value:
 *   the engine's default (0.005 and 0.01; Beamer's published 1/14 and 1/24 lose here: see the measurements).
 * The launches are enqueued ahead of the host, 8 steps at first and up to 32 at a time: every step is enqueued as three
 * launches (queue rebuild, top-down, bottom-up) that return at once unless the device-side control block says the step
 * runs in their direction, plus one small launch that closes the step; the host joins in once per batch.
 * SH_EINVAL: NULL arguments, rows < 0, max_levels < 1, a NaN share, aliasing.  SH_ESHAPE: row_ptr[0] != 0,
 * row_ptr[rows] != nnz or a row_ptr that decreases, vectors shorter than rows.  All are reported before any device work.
 * NOT covered: the other semirings, several independent sources per call (that is sh_bits_iterate), row pieces
 * (sh_spmv_step_pieces), the multi-GPU driver and the C++ harness apps (their output is the reference's 0/1 vector).
 */
typedef struct sh_bfs_graph sh_bfs_graph;
int sh_bfs_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_bfs_graph **out);
int sh_bfs_graph_free(sh_engine *e, sh_bfs_graph *g);
int sh_bfs_graph_footprint(const sh_bfs_graph *g, uint64_t *device_bytes);
int sh_bfs_graph_edges(const sh_bfs_graph *g, int64_t *edges);
int sh_bfs_levels(sh_engine *e, sh_bfs_graph *g, const sh_vec *x0, sh_vec *level, sh_vec *parent, int32_t max_levels,
                  double up_share, double down_share, int32_t *depth, int64_t *reached, int32_t *complete,
                  int32_t *mode_per_level, int64_t *size_per_level, int64_t *edges_per_level, uint64_t *ns_per_level,
                  uint64_t *total_ns);

/* ---- bucketed SSSP with distances and canonical predecessors: extends the SSSP loop of HarnessSSSP::executeRun
 *      (app/sssp.cpp:97-176) and Harness::executeKernel (inc/harness.h:149-195).  The reference's SSSP is Bellman-Ford
 *      as an SpMV loop on the (min,+) semiring: every launch reads the whole matrix, and a run takes as many launches as
 *      the longest shortest path has edges; it has no counterpart of the calls below.  sh_sssp is an SSSP that is an
 *      algorithm of its own: a bucketed, push-based label-correcting search (near-far: Davidson, Baxter, Garland, Owens,
 *      IPDPS 2014; delta-stepping: Meyer, Sanders 2003) whose work is proportional to the edges it relaxes, and which
 *      answers, on request, THROUGH WHICH vertex every distance was reached.
 *
 *      An EDGE c -> r of weight w = |a| exists when row r stores an entry with column c, 0 <= c < rows, and a value a
 *      whose magnitude is finite.  A stored zero IS an edge, of weight 0 ((min,+) is unlike (or,and) here); an infinite
 *      weight is no edge (under SH_MIN_PLUS_F32 it can never bring a word below FLT_MAX); NaN weights are outside the
 *      contract, as for sh_iterate; parallel edges are legal.  The START is d0[v] = |x0[v]| (no NaN; an infinite start
 *      counts as FLT_MAX, which is what sh_iterate's first launch makes of it): any non-negative vector is legal -- one
 *      source at 0, several sources, sources with offsets; a vertex with d0 = FLT_MAX is not a source.
 *        dist      = the greatest vector F <= d0 with F[r] <= fl32(F[c] + w) for every edge; equivalently the minimum over
 *                    all paths of the path's length added up left to right in float32 from d0 of its first vertex
 *                    (tests/minplus_ref.py gives the induction).  fl32 is monotone, so this vector is unique: ANY sequence
 *                    of relaxations dist[r] = min(dist[r], fl32(dist[c] + w)) that starts at d0 and ends when no edge
 *                    improves anything arrives at it, whatever the order, bucket width or queue contents.  It is
 *                    therefore, bit for bit, what sh_iterate(SH_MIN_PLUS_F32, alpha = 0, beta = 0, y0 = x0) leaves when
 *                    it runs with a delta so small that it stops only when nothing changes.
 *        pred[v]   = -1 when bits(dist[v]) == bits(d0[v]) (the start value stands: v is a source, or unreached, or
 *                    nothing beat its offset); otherwise the SMALLEST c with an edge c -> v and
 *                    bits(fl32(dist[c] + w)) == bits(dist[v]) -- at a fixed point one exists.  Canonical, so comparable
 *                    with ==; computed by one row-parallel pass after the search, and only when `pred` is given (the
 *                    search itself carries no predecessor atomics).  pred is a FOREST whenever fl32(dist[c] + w) > dist[c]
 *                    on every edge used; zero weights, or weights below half an ulp of the distance, can tie a vertex to
 *                    one that is no nearer and close a cycle.
 *        *reached  = vertices with dist < FLT_MAX.  *complete = 1 when the search ran out of work; 0 when max_rounds
 *                    rounds were used up first: dist then satisfies fixed point <= dist <= d0 elementwise, every word is
 *                    the rounded length of a real path, and pred is not written.
 *        *rounds, *buckets (how often the threshold advanced) and *relaxed (edges looked at) are informational, as are
 *                    the per-round arrays: the relaxations of one round race through atomic minima, so these counts may
 *                    differ from run to run.  One statement holds for every complete run:
 *                    *relaxed >= the sum of the out-degrees of the reached vertices.
 *      delta is the bucket width: > 0 is used as given; +Inf means one bucket (a frontier push Bellman-Ford); <= 0 means
 *      the engine's default, computed at handle creation as 32 * (mean weight) / (mean out-degree) = 32 * (sum of the
 *      weights / edges) * (rows / edges) (1 if that is 0) and readable through sh_sssp_graph_delta; NaN gives SH_EINVAL.
 *      The result does not depend on delta.
 *
 *      Measured on an MI355X (DESIGN.md "6f Bucketed SSSP", profiles/sssp_*.json): NOTHING YET.  tools/sssp_bench.py
 *        (against sh_iterate(SH_MIN_PLUS_F32) under the matrix' default plan and sh_iterate_frontier at its default share,
 *        on the 2048 x 2048 grid, the 170 998-row matrix, R-MAT-23 and the power-law 10 M / 200 M matrix) has not been run,
 *        so there is no table, the factor 32 of the default width is Davidson et al.'s starting point and not the outcome
 *        of a sweep, and profiles/sssp_*.json do not exist.  What is known from sh_bfs_levels, whose control this follows:
 *        a round is four dependent launches and costs 16 to 25 us at least, so a matrix whose sh_iterate launch is cheaper
 *        than that cannot win by rounds alone, and R-MAT-23 (10 launches of 0.3 ms) has 134 M atomic relaxations to pay for.
 *        Rule: call it when you need predecessors, or a start vector's exact fixed point without choosing a delta.  For
 *        distances alone sh_iterate stays the measured path until the bench has been run; the expected gain is on grids,
 *        meshes and road-like graphs (thousands of dense launches), the expected loss on small matrices and fat power-law graphs.
 *
 * sh_sssp_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The matrix is square (rows x rows);
 * val holds float32 bit patterns; col_idx outside [0, rows) and infinite values are legal and are no edges.  The handle
 * holds on the device: the out-edges by source vertex (out_ptr[rows + 1], out_row[edges], out_w[edges] = |a|, order inside
 * one list unspecified), the in-edges by row (in_ptr[rows + 1], in_col[edges], in_w[edges], stored order of the survivors
 * kept), one stamp word per vertex, two near lists and two far lists of `rows` entries (a vertex sits in a list at most
 * once, so no list can overflow on any input), two lists of pieces of long out-lists, the pieces of long rows, a control
 * block.  Built on the device (flag per entry, exclusive scan, compaction; column histogram, scan, scatter; a reduction
 * for the mean weight).  rows == 0 gives a valid handle.  Freeing NULL is SH_OK.
 * sh_sssp_graph_footprint: device bytes held =
 *     8 * (rows + 1) + 16 * edges + 20 * rows + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 22528.
 * sh_sssp_graph_edges: the entries kept as edges.  sh_sssp_graph_delta: the default bucket width (0 for a graph without edges).
 *
 * sh_sssp: dist (float32) and pred (int32, may be NULL): vectors of >= rows elements; `rows` elements of each are
 * overwritten, no more (pred only by a complete run: a run cut short leaves every word of pred as it was); x0 is only
 * read (`rows` elements, no more); dist and pred must not alias x0 or each other.  g may serve any number of calls, one at
 * a time.  max_rounds >= 1.  A ROUND relaxes the out-edges of every vertex of the near list; when the list ran empty the
 * next round opens by moving the threshold to the end of the bucket that holds the smallest far distance (empty buckets
 * cost no round) and carrying over what falls below it.  The per-round arrays (each may be NULL) have capacity max_rounds:
 * size_per_round = vertices relaxed from, edges_per_round = edges looked at, ns_per_round / total_ns = device time
 * (hipEvent) as elsewhere; total_ns also holds the set-up launch and the predecessor pass.
 * The rounds are enqueued ahead of the host, 8 at first and up to 32 at a time: every round is four launches (the split
 * in two phases, the relaxation, one small launch that closes the round) that return at once unless the device-side
 * control block says they have work; the host reads the control block once per batch.  No kernel ever waits for another
 * kernel's write.
 * SH_EINVAL: NULL arguments, rows < 0, nnz < 0, max_rounds < 1, a NaN delta, aliasing.  SH_ESHAPE: row_ptr[0] != 0,
 * row_ptr[rows] != nnz or a row_ptr that decreases, vectors shorter than rows.  All are reported before any device work.
 * NOT covered: the other semirings, several independent start vectors per call (that is sh_iterate_multi), row pieces
 * (sh_spmv_step_pieces), the multi-GPU driver and the C++ harness apps (their output stays the reference's vector).
 */
typedef struct sh_sssp_graph sh_sssp_graph;
int sh_sssp_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const void *val, sh_sssp_graph **out);
int sh_sssp_graph_free(sh_engine *e, sh_sssp_graph *g);
int sh_sssp_graph_footprint(const sh_sssp_graph *g, uint64_t *device_bytes);
int sh_sssp_graph_edges(const sh_sssp_graph *g, int64_t *edges);
int sh_sssp_graph_delta(const sh_sssp_graph *g, double *delta);
int sh_sssp(sh_engine *e, sh_sssp_graph *g, const sh_vec *x0, sh_vec *dist, sh_vec *pred, double delta,
            int32_t max_rounds, int32_t *rounds, int32_t *buckets, int64_t *reached, int32_t *complete,
            int64_t *relaxed, int64_t *size_per_round, int64_t *edges_per_round, uint64_t *ns_per_round,
            uint64_t *total_ns);

/* ---- strongly connected components by trim, pivot and colouring: extends the SCC loop of HarnessSCC::executeRun
 *      (app/scc.cpp:96-176) and Harness::executeKernel (inc/harness.h:149-195).  The reference's SCC app is an SpMV loop
 *      on the (max,min) semiring; on scc_normalise'd input it leaves a label vector that is NOT the partition into
 *      strongly connected components, and the reference has no counterpart of the calls below.  sh_scc computes that
 *      partition: trimming (Fleischer, Hendrickson, Pinar 2000), one forward-backward round from a pivot, then
 *      colouring rounds (Orzan 2004), scheduled as in Slota, Rajamanickam, Madduri (IPDPS 2014).
 *
 *      The edge rule is that of sh_bfs_levels: an EDGE c -> r exists when row r stores an entry with column c,
 *      0 <= c < rows, and a value whose 32 bits are not all zero.  Self-loops and parallel edges are legal and change nothing.
 *        comp[v]   = the largest u such that v reaches u and u reaches v (v itself counts): canonical, so comparable
 *                    with ==.  It is -1 only where an incomplete run (*complete == 0: max_steps used up) had not settled
 *                    v; every word that is not -1 is final and right.
 *        *components = the number of v with comp[v] == v; *settled = the number of v with comp[v] >= 0; *trimmed = the
 *                    vertices settled by trim rounds.
 *      The result does not depend on trim, pivot, the schedule or the run.
 *
 *      A STEP is one sweep over a work list: a trim sweep, a propagation sweep or a claim sweep (and, once per round that
 *      is no trim round, the sweep that seeds its colours; once per pivot round, the sweep that writes its label).  A
 *      ROUND is a maximal run of steps of one kind that settles vertices; kind_per_round is 0 (trim), 1 (pivot) or
 *      2 (colouring).  The schedule is fixed, so kind_per_round and size_per_round are the same in every run.  LIVE means
 *      not settled; edges count only between live vertices, and self-loops never count.
 *        1. If trim != 0, a TRIM ROUND: repeatedly settle every live vertex with no live in-neighbour or no live
 *           out-neighbour as its own component (comp[v] = v), until none is left.  The set it removes is unique (a
 *           closure).  A trim round that settles nothing is not recorded.
 *        2. If live vertices remain and pivot != 0, a PIVOT ROUND, at most once per call: p = the live vertex with the
 *           largest (stored in-list length) x (stored out-list length) as uint64, ties to the largest index; mark what p
 *           reaches through live vertices; from p claim backwards along in-lists inside the marked set.  The claimed set
 *           is p's component and gets the largest index in it as its label.
 *        3. Otherwise a COLOURING ROUND: every live v starts with colour v; colours propagate forwards along live edges by
 *           atomic max until nothing changes (colour[u] is then the largest live index that reaches u); the roots are
 *           the v with colour[v] == v; from all roots at once, claim backwards along in-lists any live c whose colour
 *           equals that of the claimed vertex it has an edge to.  The claimed vertices get their colour as label.
 *        4. After every pivot or colouring round go to 1.  Stop when no vertex is live.
 *      Why that is right: a path between two vertices of one component stays inside it, so removing whole components
 *      leaves the others intact in the live subgraph.  A root v is the largest index of its component (every member
 *      reaches v).  c is claimed iff c reaches v (the claim) and v reaches c (the colour), and every vertex on a path inside
 *      v's component has colour v.  Every colouring round settles at least the component of the largest live index.
 *      Worst cases: a descending chain of k components takes k colouring rounds (and a propagation sweep per hop in each:
 *      the directed path n - 1 -> ... -> 0 without trim takes n rounds and about n * n / 4 sweeps); a directed path takes
 *      rows / 2 trim sweeps.  max_steps bounds the call.
 *
 *      Measured on an MI355X (DESIGN.md "6g Strongly connected components", profiles/scc_grid2048.json, scc_scircuit.json, scc_rmat23.json;
 *        tools/scc_bench.py, one process per matrix, arms alternating, 5 rounds, device time in us as median (min-max);
 *        Tarjan = wall time of hostlib.scc_labels, two BFS = two sh_bfs_levels calls from the pivot on the matrix and on
 *        its transpose):
 *        - 2048 x 2048 grid (4 194 304 rows, 16 769 024 edges): trim + pivot 255 608 us (241 168-271 066), 8190 steps = 3.66 of Tarjan's 69 869 (66 127-71 147);
 *          pivot round 255 502 = 1.30 of two BFS 196 965 (196 492-200 049); trim + colouring 1 531 543 = 21.92 of Tarjan
 *        - 170 998-row matrix (scircuit stand-in) (170 998 rows, 958 936 edges): trim + pivot 2 296 us (2 180-2 315), 36 steps = 0.12 of Tarjan's 19 602 (14 995-31 996);
 *          pivot round 2 167 = 2.37 of two BFS 914 (849-930); trim + colouring 4 843 = 0.25 of Tarjan
 *        - R-MAT-23 (8 388 608 rows, 134 217 728 edges): trim + pivot 34 608 us (34 577-34 676), 19 steps = 0.010 of Tarjan's 3 442 346 (3 369 227-3 467 730);
 *          pivot round 28 693 = 22.09 of two BFS 1 299 (1 294-1 311); trim + colouring 48 855 = 0.014 of Tarjan
 *        A step with next to nothing to do costs 29-33 us (medians of three runs over 20 699 steps; single runs 23.5-40.2):
 *        eight launches, seven of them empty, against 16 to 25 us of a sh_bfs_levels step.  The power-law 10 M / 200 M
 *        matrix has no run on record.
 *        Rule: call it, with trim and pivot on (the defaults), on graphs of small diameter: R-MAT-23 is settled 100
 *        times faster than by the host Tarjan, the 170 998-row matrix 8 times.  Never turn pivot off when a giant
 *        component is expected (the colouring round costs 1.5 to 6 times the pivot round).  Do NOT call it on high-diameter
 *        graphs -- grids, meshes, road networks: about 31 us per hop of the diameter, twice over; the 2048 x 2048 grid
 *        LOSES to the host Tarjan by 3.7 and by 22 without the pivot round -- nor on long chains of components.  The pivot
 *        round itself loses to the two-BFS yardstick everywhere, by 22 on R-MAT-23 (it pushes along every edge with
 *        atomics where the BFS goes bottom-up): for one vertex' reach alone call sh_bfs_levels.  In a trim sweep a list
 *        longer than 32 entries is searched by one wave without pieces: a hub whose neighbours are all settled costs that
 *        wave a walk of the whole list.  The power-law matrix is unmeasured.
 *
 * sh_scc_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The matrix is square (rows x rows);
 * col_idx outside [0, rows) and stored zeros are legal and are no edges.  The handle holds on the device: the edge pattern
 * by rows and its transpose as sh_bfs_graph does, one colour and one stamp word per vertex, two work lists and the trim's
 * candidate list of `rows` entries (a vertex enters a list at most once per sweep, so no list can overflow on any input),
 * two lists of pieces of long out-lists and two of long in-lists, the pieces of long rows, a control block.
 * rows == 0 gives a valid handle.  Freeing NULL is SH_OK.
 * sh_scc_graph_footprint: device bytes held =
 *     8 * (rows + 1) + 8 * edges + 20 * rows + 32 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 34816.
 * sh_scc_graph_edges: the entries kept as edges.
 *
 * sh_scc: comp: an int32 vector of >= rows elements; `rows` elements are overwritten, no more.  g may serve any number
 * of calls, one at a time.
 * max_steps >= 1.  The per-round arrays (each may be NULL) have capacity max_steps; one entry per recorded round:
 * size_per_round = vertices the round settled; steps_per_round, edges_per_round (edges looked at), ns_per_round and
 * total_ns are informational (the sweeps race, so their number may differ from run to run); ns_per_round / total_ns are
 * device time (hipEvent) as elsewhere, total_ns also holds the set-up launch and the trim rounds that settled nothing.
 * The steps are enqueued ahead of the host, 8 at first and up to 32 at a time: every step is a fixed set of eight launches
 * (trim in two phases, pivot choice, seed, propagation, claim, label, one small launch that closes the step) that return
 * at once unless the device-side control block gives them work; the host reads the control block once per batch.
 * No kernel ever waits for another kernel's write.
 * SH_EINVAL: NULL arguments, rows < 0, nnz < 0, max_steps < 1.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a
 * row_ptr that decreases, comp shorter than rows.  All are reported before any device work.
 * NOT covered: the other semirings, row pieces (sh_spmv_step_pieces), the multi-GPU driver, the C++ harness apps
 * (scc_harness keeps the reference's vector), a serial tail for long chains.  (What hangs together regardless of direction, the weakly connected
 * components, is sh_wcc's: below and DESIGN.md 6h.)
 */
typedef struct sh_scc_graph sh_scc_graph;
int sh_scc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_scc_graph **out);
int sh_scc_graph_free(sh_engine *e, sh_scc_graph *g);
int sh_scc_graph_footprint(const sh_scc_graph *g, uint64_t *device_bytes);
int sh_scc_graph_edges(const sh_scc_graph *g, int64_t *edges);
int sh_scc(sh_engine *e, sh_scc_graph *g, sh_vec *comp, int32_t trim, int32_t pivot, int32_t max_steps,
           int64_t *components, int64_t *settled, int64_t *trimmed, int32_t *rounds, int32_t *steps, int32_t *complete,
           int32_t *kind_per_round, int64_t *size_per_round, int32_t *steps_per_round, int64_t *edges_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns);

/* ---- weakly connected components by hooking roots and pointer jumping: extends the SCC loop of HarnessSCC::executeRun
 *      (app/scc.cpp:96-176) and Harness::executeKernel (inc/harness.h:149-195); the reference has no counterpart of the
 *      calls below.  sh_wcc answers which vertices hang together at all: hooking and pointer jumping (Shiloach, Vishkin
 *      1982) with neighbour sampling and a skip of the largest tree (Sutton, Ben-Nun, Barak, "Afforest", IPDPS 2018).  It
 *      is the first search here that does not pay per hop of the diameter.
 *
 *      The edge rule is that of sh_bfs_levels / sh_scc: row r storing column c with 0 <= c < rows and a value whose 32
 *      bits are not all zero is an EDGE.  Here its direction is ignored.  Self-loops, parallel edges, stored zeros and
 *      columns outside the matrix are legal and change nothing.
 *        comp[v]     = the largest vertex index of v's weak component (the convention of sh_scc): canonical, so
 *                      comparable with ==.  On a pattern that holds c -> r whenever it holds r -> c, sh_wcc's comp equals
 *                      sh_scc's.  After an incomplete run (*complete == 0: max_rounds used up) comp is -1 EVERYWHERE,
 *                      because a half-built forest is not a partition; the handle is still good for another call.
 *        *components = the number of v with comp[v] == v; *skipped = the number of vertices whose lists the full rounds
 *                      did not walk (0 when sample == 0).
 *      The result does not depend on sample, the schedule or the run.
 *
 *      State: one parent word p[v] per vertex, p[v] >= v always, so there are no cycles and a root (p[r] == r) is the
 *      largest index of its tree.  A HOOK is a compare-and-swap on a root: p[lo] goes from lo to hi, lo < hi; a JUMP is
 *      p[v] = p[p[v]].  So trees only ever merge, never split; no pointer of a non-root is ever raised by an atomic max.
 *      A ROUND is one fixed set of launches; kind_per_round is 0 (a sampling round) or 1 (a full round).
 *        1. p[v] = v.
 *        2. SAMPLING ROUNDS j = 0 .. sample - 1: every vertex hooks along the j-th stored edge of its row, if it has one;
 *           then up to 6 jumping launches over all rows (at most 8 jumps per vertex each), each of which returns at once
 *           unless the one before it changed a pointer.
 *        3. PICK AND COMPACT, only if sample > 0, in front of the first full round: L = the most frequent parent among the
 *           1024 vertices v = i * rows / 1024, ties to the larger index (deterministic for a given forest; a sample, so it
 *           may pick any tree, and the result never depends on which).  S = { v : p[v] == L } is fixed here, once.  The
 *           vertices outside S are compacted into one work list, their long in-lists and long out-lists into two piece
 *           lists.  With sample == 0, S is empty and the list is every vertex.
 *        4. FULL ROUNDS: for every entry of the in-lists AND of the out-lists of the work list's vertices, hook the two
 *           ends (an edge with one end in S is stored in the row of either end and only the other end walks; edges inside
 *           S are never looked at); then the jumping launches, over all rows.  A hook climbs from the smaller of the two
 *           ancestors it holds, and retries after a failed compare-and-swap, at most 8 times in all; an entry it could
 *           not settle is left to the next round and counted, so the run cannot end over it.
 *        5. Stop after a full round that found both ends of every walked entry under one parent, hooked nothing and
 *           jumped nothing.  comp[v] = p[v].
 *      Why that is right: pointers never leave a component.  The last round wrote nothing, so what it saw is one state:
 *      every tree a star, every walked edge with both ends under one root.  S sits in one tree.  So a component is one
 *      star, and its root is its largest index.
 *      Worst cases: the number of rounds grows with log(rows) while the lanes' races are won at random, not with the
 *      diameter (a path of 65 536 vertices: 2 to 9 rounds).  Hooking on roots only needs many rounds when ONE root is
 *      wanted by many larger ones and the smallest keeps winning: a vertex of smallest index whose k neighbours hook in
 *      ascending order settles 8 of them per round, k / 8 rounds (not seen in a run: which lane wins is arbitrary, and
 *      the wanted set then about halves per try).  Every tree of larger index that joins a star re-roots it: all its
 *      members jump again.  A round's jumping launches halve every depth six times at least; what is left is jumped in
 *      the next round.  Every round costs its ten launches, the empty ones included.  max_rounds bounds the call.
 *
 *      Measured on an MI355X (DESIGN.md "6h Weakly connected components", profiles/wcc_scircuit.json; tools/wcc_bench.py,
 *        one process per matrix, arms alternating, 5 rounds, device time in us as median (min-max); union-find = wall
 *        time of hostlib.wcc_labels; sh_scc with trim and pivot on the matrix plus its transpose):
 *        - 170 998-row matrix (scircuit stand-in) (170 998 rows, 958 936 edges, one component): sample 0: 303 us
 *          (286-345), 2 rounds; sample 1: 326 (320-328), 3 rounds; sample 2: 218 (208-248), 4 rounds, 170 969 vertices
 *          skipped, 272 987 entries looked at instead of 3 835 744 = 0.053 of the union-find's 4 135 (4 008-4 152);
 *          sample 4: 266 (254-269), 6 rounds.  On the symmetric pattern (1 917 872 edges): sh_wcc sample 2 207
 *          (186-234) = 0.096 of sh_scc's 2 161 (2 116-2 164, 18 steps).
 *        - the 2048 x 2048 grid and R-MAT-23 have no run on record: unmeasured.
 *        From the tests (single runs): a path of 65 536 vertices 2-9 rounds, 87-420 us; the 128 x 128 grid 2-3 rounds.
 *        A round with next to nothing to do costs about 25 us (ten launches).
 *        Rule: for what hangs together regardless of direction call sh_wcc, not sh_scc on a symmetrised pattern: on the
 *        one matrix measured it is 10 times faster on the same input and takes half the device memory.  Keep the
 *        default sample = 2: it is the fastest of 0, 1, 2, 4 there (one sampled neighbour leaves the largest tree too
 *        small to skip, four cost two more rounds than they save).  A call is at least sample + 1 rounds of about 25 us each, whatever
 *        the graph.  Whether the grid wins against the host
 *        union-find and what the skip saves on R-MAT-23 is not known: both are unmeasured.
 *
 * sh_wcc_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The matrix is square (rows x rows).
 * The handle holds on the device: the edge pattern by rows and its transpose as sh_bfs_graph does, one parent word per
 * vertex, one work list of `rows` entries (a vertex enters it at most once per call, so it cannot overflow on any input),
 * one list of pieces of long in-lists and one of long out-lists, the pieces of long rows, a control block.
 * rows == 0 gives a valid handle.  Freeing NULL is SH_OK.
 * sh_wcc_graph_footprint: device bytes held =
 *     8 * (rows + 1) + 8 * edges + 8 * rows + 16 * (edges / 1024 + 1) + 8 * (edges / 2048 + 1) + 34816.
 * sh_wcc_graph_edges: the entries kept as edges.
 *
 * sh_wcc: comp: an int32 vector of >= rows elements; `rows` elements are overwritten, no more.  g may serve any number
 * of calls, one at a time.
 * sample >= 0: the number of stored neighbours per vertex that the sampling rounds look at (the Python binding's default
 * is 2).  max_rounds >= 1.  The per-round arrays (each may be NULL) have capacity max_rounds, one entry per round:
 * hooks_per_round (compare-and-swaps won), jumps_per_round (pointers changed), edges_per_round (entries looked at),
 * ns_per_round, total_ns and *rounds itself are informational: the lanes race, so they may differ from run to run.
 * ns_per_round / total_ns are device time (hipEvent) as elsewhere; total_ns also holds the set-up and the labelling launch.
 * The rounds are enqueued ahead of the host, 8 at first and up to 32 at a time: every round is a fixed set of ten launches
 * (sampling hooks, pick and compaction, the full walk, six jumping launches, one small launch that closes the round) that
 * return at once unless the device-side control block gives them work; the host reads the control block once per batch.
 * No kernel ever waits for another kernel's write, and no lane spins on a word until another lane writes it.
 * SH_EINVAL: NULL arguments, rows < 0, nnz < 0, sample < 0, max_rounds < 1.  SH_ESHAPE: row_ptr[0] != 0,
 * row_ptr[rows] != nnz or a row_ptr that decreases, comp shorter than rows.  All are reported before any device work.
 * NOT covered: the multi-GPU driver, row pieces (sh_spmv_step_pieces), the C++ harness apps, component sizes or a
 * histogram, incremental updates.
 */
typedef struct sh_wcc_graph sh_wcc_graph;
int sh_wcc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_wcc_graph **out);
int sh_wcc_graph_free(sh_engine *e, sh_wcc_graph *g);
int sh_wcc_graph_footprint(const sh_wcc_graph *g, uint64_t *device_bytes);
int sh_wcc_graph_edges(const sh_wcc_graph *g, int64_t *edges);
int sh_wcc(sh_engine *e, sh_wcc_graph *g, sh_vec *comp, int32_t sample, int32_t max_rounds,
           int64_t *components, int64_t *skipped, int32_t *rounds, int32_t *complete,
           int32_t *kind_per_round, int64_t *hooks_per_round, int64_t *jumps_per_round, int64_t *edges_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns);

/* ---- exact triangle counts, per vertex and in total, by intersecting forward lists: extends the graph handles made from
 *      the CSR arrays alone (sh_bfs_graph_create ... sh_wcc_graph_create above), which extend the loop of
 *      HarnessSCC::executeRun (app/scc.cpp:96-176) and Harness::executeKernel (inc/harness.h:149-195); the reference
 *      has no counterpart of the calls below.  In semiring words the total is the sum of (L . L) o L on (+,x), L the
 *      oriented pattern; the mask makes the product an intersection of two sorted lists, not another SpMV.
 *
 *      The edge rule is that of sh_bfs_levels / sh_scc / sh_wcc: row r storing column c with 0 <= c < rows and a value
 *      whose 32 bits are not all zero is an entry that counts.  The graph is the SIMPLE UNDIRECTED graph under those
 *      entries: {u, v} with u != v is one edge if either row stores the other, once or many times.  Self-loops, parallel
 *      entries, stored zeros and columns outside the matrix are legal and change nothing.  M = the number of such edges.
 *        tri[v]      = the number of triangles {v, a, b} of that graph, an unsigned 64-bit count per vertex.
 *        deg[v]      = the degree of v in that graph (int32).  The local clustering coefficient is then
 *                      2 * tri / (deg * (deg - 1)), one line for the caller; there is no call for it.
 *        *triangles  = the number of triangles = (the sum of tri[v]) / 3.
 *      The result does not depend on order, the schedule or the run: counts are integers and integer addition is
 *      associative, so every comparison is ==.
 *
 *      order = 0 orients every edge from the smaller index to the larger; order = 1 (the Python binding's default) from
 *      the smaller (deg, index) pair to the larger.  N+(v), the forward list of v, holds the ends of the edges that leave
 *      v, strictly ascending by index.  Under order = 1 every forward list holds at most sqrt(2M) entries: the
 *      out-neighbours of v all have degree >= deg(v) >= |N+(v)|, so the degrees of those |N+(v)| vertices alone add up to
 *      at least |N+(v)|^2, and all degrees add up to 2M.  Both orders give the same tri.
 *      Schedule: a fixed number of launches, no host loop.  Every triangle has one lowest vertex a and one middle vertex
 *      b in the orientation's order; it is found once, at the forward edge a -> b, as an element c of both N+(a) and
 *      N+(b).  The work item is a source vertex a with its whole forward list, in one of three classes by its length n:
 *      n <= 8: one lane (every other c of N+(a) is bisected into N+(b) in memory); 8 < n <= 512: one wave (N+(a) staged
 *      in LDS once, every N+(b) streamed with coalesced loads, each entry bisected into the staged list); n > 512: one
 *      workgroup, N+(a) staged in chunks of at most 2048 entries, every N+(b) of the whole list streamed against each
 *      chunk.  A list of any length goes through the chunks: there is no further path for longer lists.
 *      Per found c one 64-bit add to tri[c]; the hits of an edge a -> b are counted across the wave and added once to
 *      tri[b], those of all of a's edges once to tri[a]; totals go per workgroup into partial sums that a last small launch
 *      adds up.  With tri == NULL the adds to tri are not compiled in.
 *      Why that is right: the order is total, so a triangle's vertices are a < b < c in one way; its edges are then b in
 *      N+(a), c in N+(a), c in N+(b) and in no other list; the count at edge x -> y sees z in both N+(x) and N+(y), which
 *      needs x < y < z: the edge a -> b alone, and c stands once in either list.  No kernel ever waits for another
 *      kernel's write, and every loop is bounded by a list length.
 *      Worst cases: under order = 0 a hub of smallest index has its whole row as its forward list (one workgroup walks
 *      it, against every neighbour's list, once per chunk of 2048).  A dense clique costs its n^3 / 6 hits under either
 *      order, each an atomic add when tri is wanted.  A wave takes the b of its list one after the other: forward lists
 *      of a few entries leave most of its lanes idle.
 *
 *      Measured on an MI355X (DESIGN.md "6i Triangle counting"; tools/tri_bench.py, one process per matrix, arms
 *        alternating, 5 rounds, device time against the wall time of hostlib.triangle_counts): no run is on record.
 *        The 170 998-row matrix (scircuit stand-in), R-MAT-18 and the 2048 x 2048 grid are all unmeasured, and so is
 *        the time of K_2400 in the tests.
 *        Rule: the numbers support no rule yet.  By construction order = 1 bounds every forward list by sqrt(2M) and
 *        order = 0 does not; pass tri == NULL when only the total is wanted.  Whether a call beats the host's forward
 *        algorithm, and by how much order = 1 beats order = 0, is unmeasured.
 *
 * sh_tri_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The matrix is square (rows x rows).
 * order: 0 or 1, see above.  The handle holds on the device: fwd_ptr[rows + 1], fwd_col[M], deg[rows] and a control block
 * (with the workgroups' partial sums); nothing else, and no transpose.  rows == 0 gives a valid handle.  Freeing NULL is
 * SH_OK.  The build runs on the device, once: the entries that count and are no self-loops become 64-bit keys
 * (min << bits | max, bits = those of rows - 1), a radix sort over 2 * bits bits, the first key of every run is an edge,
 * deg is a histogram over both ends, the oriented keys (src << bits | dst) are sorted again and the row starts taken
 * from them.  While it runs the build needs 4 * (rows + 1) + 16 * nnz + 8 bytes for the arrays as given, their flags and
 * scan, 16 bytes per surviving entry for the keys and the sorted keys, and the sort's own scratch (rocPRIM: about one
 * more copy of the keys); all of it is released before the call returns.  nnz is bounded as for the other handles.
 * sh_tri_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 4 * rows + 4 * edges + 33024.
 * sh_tri_graph_edges: M.  sh_tri_graph_max_forward: the length of the longest forward list.
 *
 * sh_tri: tri: NULL, or a vector of >= 2 * rows four-byte elements, 8-byte aligned, read as `rows` little-endian uint64
 * (as the `words` per vertex of sh_bits_*: all elements are still 4 bytes); 2 * rows elements are overwritten, no more.
 * With tri == NULL the call gives the total only and does not pay for the per-vertex adds.  deg: NULL, or an int32 vector
 * of >= rows elements; `rows` elements are overwritten, no more.  A per-vertex count above 2^32 needs a vertex in more
 * than 4.29e9 triangles; no test reaches that:
 * the high word of tri[v] is untested beyond being zero.  *triangles above 2^31 is tested (K_2400).
 * *probes (may be NULL) is informational: the list entries the count looked at, each time it looked (the entries of N+(a)
 * once, every streamed entry of an N+(b) once, every entry a bisection compared with).  *total_ns (may be NULL) is device
 * time (hipEvent) as elsewhere.  g may serve any number of calls, one at a time.
 * SH_EINVAL: NULL arguments (engine, graph, triangles, out, the arrays), rows < 0, nnz < 0, an order other than 0 or 1, a
 * tri that is not 8-byte aligned.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases, tri
 * shorter than 2 * rows, deg shorter than rows.  All are reported before any device work, with the buffers untouched.
 * NOT covered: per-edge support and k-truss, the multi-GPU driver, row pieces (sh_spmv_step_pieces), the C++ harness
 * apps, incremental updates.  (Per-edge support and truss numbers on the same graph are sh_truss's, below.)
 */
typedef struct sh_tri_graph sh_tri_graph;
int sh_tri_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, int32_t order, sh_tri_graph **out);
int sh_tri_graph_free(sh_engine *e, sh_tri_graph *g);
int sh_tri_graph_footprint(const sh_tri_graph *g, uint64_t *device_bytes);
int sh_tri_graph_edges(const sh_tri_graph *g, int64_t *edges);            /* M */
int sh_tri_graph_max_forward(const sh_tri_graph *g, int64_t *entries);    /* the longest forward list */
int sh_tri(sh_engine *e, sh_tri_graph *g, sh_vec *tri, sh_vec *deg,
           uint64_t *triangles, uint64_t *probes, uint64_t *total_ns);

/* ---- core numbers (k-core decomposition) and the degeneracy, by parallel peeling: extends the graph handles made from
 *      the CSR arrays alone (sh_bfs_graph_create ... sh_tri_graph_create above), which extend the loop of
 *      HarnessSCC::executeRun (app/scc.cpp:96-176) and Harness::executeKernel (inc/harness.h:149-195); the reference
 *      has no counterpart of the calls below.
 *
 *      The edge rule is word for word sh_tri's: row r storing column c with 0 <= c < rows and a value whose 32 bits are
 *      not all zero is an entry that counts.  The graph is the SIMPLE UNDIRECTED graph under those entries: {u, v} with
 *      u != v is one edge if either row stores the other, once or many times.  Self-loops, parallel entries, stored
 *      zeros, columns outside the matrix and direction are legal and change nothing.  M = the number of such edges.
 *        core[v]      = the core number of v: the largest k such that v lies in a subgraph whose vertices all have at
 *                       least k neighbours in it (int32, one per vertex).
 *        deg[v]       = the degree of v in that graph (int32), as sh_tri's.
 *        *degeneracy  = max core[v]; 0 for a graph without edges or rows.
 *        *levels      = the number of distinct values in core.
 *        *rounds      = the number of peel rounds run.
 *        *complete    = 1 if every vertex was settled within max_rounds; if 0, core holds -1 for the vertices not yet
 *                       settled and the settled ones are right (and *degeneracy, *levels speak of the settled ones).
 *      core, deg, *degeneracy and *levels do not depend on chase, the schedule or the run: a graph has one vector of core
 *      numbers and they are integers, so every comparison is ==.
 *
 *      Schedule (csrc/core.hip.h).  cur[v] is the remaining degree of v, core[v] = -1 until v is settled.  The call walks
 *      the levels k upwards and runs rounds inside a level; a round is one fixed set of four launches enqueued ahead of
 *      the host in batches (8, 16, 32, 32, ...), each of which returns at once unless the control block on the device
 *      gives it work; the host learns k, the list sizes and the end only from one readback per batch.  When the work
 *      list is empty and vertices remain, the round opens a level: one pass over all vertices takes the smallest cur
 *      among the unsettled (a minimum per workgroup, not one word hit by every wave), that minimum becomes k -- empty
 *      levels are skipped, not walked -- and a second pass puts every unsettled v with cur[v] <= k on the work list.
 *      The peel then walks the lists of the work list's vertices -- up to 8 entries one lane, up to 2048 one wave,
 *      longer ones in pieces of 2048, one wave per piece -- settles v with core[v] = k and gives every entry u with
 *      cur[u] > k one atomic decrement.  The one lane that sees the old value k + 1 owns u and appends it to the next
 *      round's list; a lane that sees an old value <= k restores it with one add.  There is no compare-and-swap and no
 *      retry.  A last small launch sums the workgroups' counts, takes the settled from the remaining, swaps the lists,
 *      records the round and finishes when nothing remains.
 *      chase > 0: a lane that owns a u whose list has at most 8 entries keeps it in hand (at most one; any other goes to
 *      the next list), and after its own walk settles u and walks u's list the same way, at most `chase` times in a
 *      row; what it still holds then goes to the next list.  The loop is bounded by chase * 8 entries per lane.  It keeps
 *      a chain from costing one round per vertex: a path of n vertices takes about n / (2 (chase + 1)) rounds instead
 *      of n / 2.
 *      What is deterministic: with chase == 0 a round's set is exactly the vertices whose remaining degree fell to <= k
 *      in the round before (in an opening round: those whose remaining degree is the smallest), so *rounds, k_per_round,
 *      size_per_round and edges_per_round are deterministic too.  With chase > 0 these records are informational -- who
 *      owns, and so who is chased, depends on the schedule -- and *rounds is never larger than with chase == 0.
 *      Why that is right: peeling is monotone -- removing more only lowers remaining degrees further.  A level ends when
 *      no unsettled vertex has cur <= k; the set settled in it is the closure of "delete a vertex of remaining degree
 *      <= k", the same in whatever order and grouping, so every level starts from one state and core[v] is the level v
 *      fell in.  If a chasing run has settled a superset A of what the run with chase == 0 has settled (B) after as many
 *      rounds, a vertex of remaining degree <= k after B's deletions has it after A's too, so it is settled in A or on A's
 *      list: one round later A still contains B.  The decrement: once the word of u has gone from k + 1 to k, it is k
 *      minus the decrements that have not restored yet and never exceeds k again, so the owner is unique, and every
 *      reader only compares with `> k`, so a transient value below k answers like k (csrc/core.hip.h has the steps).
 *      Every vertex is settled once; no kernel ever waits for another kernel's write; every loop is bounded by a list
 *      length, `rows` or chase * 8.
 *      Worst cases: the number of rounds is the depth of the peeling, not the diameter -- a path or a grid needs rounds
 *      in proportion to its side (the 128 x 128 grid: 127 rounds, one level; chasing shortens chains of short lists
 *      only).  Every non-empty level costs two passes over all vertices.  A hub's list is walked once, in pieces, when
 *      the hub is settled.
 *
 *      Measured on an MI355X (DESIGN.md "6j k-core decomposition"; tools/core_bench.py, one process per matrix, arms
 *        chase = 0 / 4 / 16 / 64 alternating, 5 rounds, device time against the wall time of hostlib.core_numbers):
 *        the 2048 x 2048 grid (4 194 304 rows, 8 384 512 edges, degeneracy 2, one level; host gold 652 ms), median
 *        (min-max) in ms and rounds: chase 0: 47.8 (47.7-48.1), 2047; 4: 58.4 (58.3-58.5), 1194; 16: 119.7 (119.1-119.8),
 *        1082; 64: 314.4 (314.0-314.7), 1039.  R-MAT-18 (262 144 rows, 3 805 085 edges, degeneracy 374, 138 levels, largest
 *        degree 25 104; host gold 312 ms): chase 0: 45.57 (45.49-45.61), 451; 4: 45.49 (45.42-45.52), 442; 16: 45.41
 *        (45.37-45.43), 442; 64: 45.47 (45.46-45.52), 442.  The handle is built in 0.06 s on either.  A round of four
 *        launches costs about 23 us however small its list is.  On the grid chasing saves rounds and loses time: its
 *        front is no chain, and a launch lasts as long as its longest chase.  On R-MAT-18 1137 vertices are chased at all.
 *        Rule: the binding's default is chase = 0, the fastest arm on the grid and no slower than any on R-MAT-18.  Pass
 *        chase > 0 only for a graph that hangs long chains of degree-2 vertices off its cores (a path of 4096: 2048
 *        rounds with chase 0, at most 2048 / (chase + 1) + 2 with it); the time of such a run is unmeasured.
 *
 * sh_core_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The matrix is square (rows x rows).
 * The handle holds on the device: adj_ptr[rows + 1] and adj_col[2M] (every list strictly ascending; no transpose: the
 * lists are symmetric), deg[rows], cur[rows], two work lists of `rows` entries (a vertex enters a list at most once per
 * call: they cannot overflow), two piece lists of 2M / 1024 + 1 places, and a control block with the workgroups' counts.
 * rows == 0 gives a valid handle.  Freeing NULL is SH_OK.  The build runs on the device, once, and shares its first half
 * with sh_tri_graph_create: the entries that count and are no self-loops become 64-bit keys (min << bits | max, bits =
 * those of rows - 1), a radix sort over 2 * bits bits, the first key of every run is an edge, deg is a histogram over
 * both ends; then every edge is written both ways (u << bits | v and v << bits | u), the 2M keys are sorted and the row
 * starts taken from them.  While it runs the build needs 4 * (rows + 1) + 16 * nnz + 8 bytes for the arrays as given,
 * their flags and scan, 16 bytes per surviving entry for the keys and the sorted keys, 32 bytes per edge for the keys
 * both ways and their sorted copy, and the sort's own scratch (rocPRIM: about one more copy of the keys); all of it is
 * released before the call returns.  nnz is bounded as for the other handles, and 2M by 2^31 - 256.
 * sh_core_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 8 * edges + 16 * rows + 16 * (2 * edges / 1024 + 1) + 34816.
 * sh_core_graph_edges: M.  sh_core_graph_max_degree: the largest degree (the length of the longest list).
 *
 * sh_core: core: an int32 vector of >= rows elements; `rows` elements are overwritten, no more.  deg: NULL, or an int32
 * vector of >= rows elements, of which `rows` are overwritten, no more.  chase >= 0 (the Python binding's default: see
 * the rule above).  max_rounds >= 1 bounds the rounds; rows + 1 can never cut a run short (the Python binding's
 * default).  The per-round arrays (capacity max_rounds; each may be NULL): k_per_round the k being peeled,
 * size_per_round the vertices taken from the round's work list, chased_per_round the vertices settled inside the launch
 * without passing through a list, edges_per_round the list entries looked at, ns_per_round device time; size + chased
 * over all rounds of a complete run is `rows`.  *total_ns (may be NULL) is device time (hipEvent) as elsewhere.  g may
 * serve any number of calls, one at a time; every call starts from cur = deg.
 * SH_EINVAL: NULL arguments (engine, graph, core, degeneracy, levels, rounds, complete, out, the arrays), rows < 0,
 * nnz < 0, chase < 0, max_rounds < 1.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases, core
 * or deg shorter than rows.  All are reported before any device work, with the buffers untouched.
 * NOT covered: the removal order / degeneracy ordering as an output, k-truss, the multi-GPU driver, row pieces
 * (sh_spmv_step_pieces), the C++ harness apps, incremental updates.  (Truss numbers on the same lists are sh_truss's, below.)
 */
typedef struct sh_core_graph sh_core_graph;
int sh_core_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const void *val, sh_core_graph **out);
int sh_core_graph_free(sh_engine *e, sh_core_graph *g);
int sh_core_graph_footprint(const sh_core_graph *g, uint64_t *device_bytes);
int sh_core_graph_edges(const sh_core_graph *g, int64_t *edges);          /* M */
int sh_core_graph_max_degree(const sh_core_graph *g, int64_t *entries);
int sh_core(sh_engine *e, sh_core_graph *g, sh_vec *core, sh_vec *deg, int32_t chase, int32_t max_rounds,
            int32_t *degeneracy, int32_t *levels, int32_t *rounds, int32_t *complete,
            int32_t *k_per_round, int64_t *size_per_round, int64_t *chased_per_round, int64_t *edges_per_round,
            uint64_t *ns_per_round, uint64_t *total_ns);

/* ---- k-truss decomposition: the triangles through every edge and its truss number, by parallel peeling ---------------
 * (the reference has no counterpart: its apps are SpMV, PageRank, BFS, SSSP and SCC label propagation; this is the third
 * piece on sh_tri's graph, after the triangles per vertex and sh_core's core numbers, and the first whose work item and
 * output are an edge)
 *
 * The graph and the edge rule are sh_tri's, word for word: the matrix is square (rows x rows); entry j of row r storing
 * column c with 0 <= c < rows counts when its 32 value bits are not all zero (a float -0.0 counts, a stored zero does
 * not); the graph is the SIMPLE UNDIRECTED graph under those entries.  Self-loops, parallel entries, stored zeros, the
 * direction of an entry and columns outside the matrix change nothing.  M is its number of edges.
 *      Edge ids: edge e, 0 <= e < M, is the e-th smallest pair (u, v) with u < v, in lexicographic order (in numpy: the
 *      sorted unique pairs); edge_u[e] and edge_v[e] make the indexing visible.
 *      support[e] = |N(u) & N(v)|, the triangles through e; the supports sum to three times the triangles.
 *      truss[e] follows Cohen's convention: the largest k such that e lies in a subgraph all of whose edges are in at
 *      least k - 2 triangles of that subgraph.  An edge in no triangle has truss 2, and every edge of K_n has truss n.
 *      truss[e] is 0 until the edge is settled, which a caller sees only after a call cut short by max_rounds.
 *      *max_truss is the largest truss number (0 when M == 0), *levels the number of distinct ones, *triangles the sum of
 *      the supports / 3.  Per round: k_per_round, size_per_round (the edges settled) and walked_per_round, the sum of
 *      min(deg u, deg v) over the round's edges -- defined so that it is deterministic, whatever the kernel skips.
 *      Truss numbers are integers and a graph has one vector of them: every comparison is ==.
 *
 *      Schedule (csrc/truss.hip.h; PKT: Kabir, Madduri 2017).  Per edge: sup[e], the remaining support; stamp[e], 0 while
 *      the edge is alive and in no list, else the round (counted from 1) whose list holds it; truss[e].  In round r an
 *      edge is current if stamp == r, gone if 0 < stamp < r, and alive otherwise (0, or r + 1: owned during this very
 *      launch; a racing reader sees either and acts the same).  Before round 1 the support pass counts, for every edge,
 *      the entries of the shorter of its ends' two lists that the longer one holds too (a bisection per entry).  Work
 *      goes by the length of that shorter list: up to 8 entries one lane, up to 2048 one wave, longer lists in pieces of
 *      2048, one wave per piece; the first two store their count, a piece does one atomic add per piece, and the total
 *      goes into a sum per workgroup, never one word hit by every wave.  A round is one fixed set of four launches
 *      enqueued ahead of the host in batches (8, 16, 32, 32, ...), each of which returns at once unless the control
 *      block on the device gives it work.  When the work list is empty and edges remain, the round opens a level: one
 *      pass takes the smallest sup among the unsettled (a minimum per workgroup), that minimum becomes s and k = s + 2
 *      -- empty levels are skipped, not walked -- and a second pass stamps every unsettled e with sup[e] <= s and puts
 *      it on the list.  The peel walks, for each current e = {u, v}, the shorter list again; an entry w with the edge
 *      e1 = {u, w} that the longer list holds too gives e2 = {v, w} (no bisection when e1 is gone).  The rule for the
 *      triangle {e, e1, e2}: if e1 or e2 is gone, nothing -- it was taken apart in an earlier round; if both are
 *      current, nothing; if only e1 is current, e2 is decremented when e < e1 and not otherwise (the same with e1 and e2
 *      swapped), so of the two current edges exactly one acts; if neither is current, both are decremented.  Every
 *      triangle costs each surviving edge one decrement.  The decrement is sh_core's: if the word is <= s, skip; else
 *      one atomic decrement; the one lane that gets the old value s + 1 owns the edge, stamps it r + 1 and appends it to
 *      the next list; a lane that gets an old value <= s restores it with one add.  There is no compare-and-swap, no
 *      retry and no waiting.  A last small launch sums the workgroups' counts, takes the settled from the remaining,
 *      swaps the lists, records the round and finishes when nothing remains.
 *      Why that is right: peeling is monotone -- removing more only lowers remaining supports further.  A level ends when
 *      no unsettled edge has sup <= s; the set settled in it is the closure of "delete an edge of remaining support
 *      <= s", the same in whatever order, so every level starts from one state and truss[e] is the level e fell in.  A
 *      round's list is exactly the edges whose remaining support fell to <= s in the round before, so *rounds and the
 *      records per round are deterministic too; there is no chase option.  Once the word of an edge has gone from s + 1
 *      to s it never exceeds s again, so the owner is unique, and every reader only compares with `> s`, so a transient
 *      value below s answers like s.  Every edge is settled once (a list of M places cannot overflow); no kernel ever
 *      waits for another kernel's write; every loop is bounded by a list length, M or 32 halvings.
 *      Worst cases: the number of rounds is the depth of the peeling -- the triangulated 128 x 128 grid needs 128 rounds
 *      for its one level.  Every non-empty level costs two passes over all edges.  An edge between two hubs costs its
 *      shorter list, bisected into the longer, in the support pass and in the round in which it is current.  A clique of
 *      n vertices costs n^3 / 2 bisections in the support pass.
 *
 *      Measured on an MI355X (DESIGN.md "6k k-truss decomposition"; tools/truss_bench.py, one process per matrix, the
 *        two arms alternating, 5 rounds, device time against the wall time of hostlib.truss_numbers in that process),
 *        median (min-max) in ms: the triangulated 2048 x 2048 grid (4 194 304 rows, 12 574 721 edges, 8 380 418
 *        triangles, every truss 3, one level; host gold 1545): 74.8 (74.6-75.1), 2048 rounds, of which the support pass
 *        0.58.  R-MAT-14 (16 384 rows, 213 008 edges, 2 836 521 triangles, max_truss 78, 65 levels, largest degree
 *        3639; host gold 1368): 302.6 (301.2-303.1), 586 rounds, the support pass 0.50.  The handle is built in 0.06 s
 *        on either.  A round of the grid costs 37 us, launch cost; a round of R-MAT-14 costs 516 us on average -- the
 *        rounds that walk hub-hub edges, one workgroup per long item, are what the call costs, not the support pass.
 *        Rule: a call is 0.05 (grid) to 0.22 (R-MAT-14) of the host's bucket algorithm.  Each round costs its four
 *        launches however small its list is, so a deep peeling on a small graph loses to the host; below which size
 *        is unmeasured, as is any R-MAT above scale 14.
 *
 * sh_truss_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The handle holds on the device:
 * adj_ptr[rows + 1], adj_col[2M] (sh_core_graph's symmetric lists, every list strictly ascending) and adj_eid[2M], the edge
 * id of every list entry; edge_u[M], edge_v[M], deg[rows], sup[M], stamp[M]; two work lists of M entries (an edge enters a
 * list at most once per call: they cannot overflow), which keep the items of the piece class at their far end, so that
 * no list of pieces is stored -- an item is cut by the SHORTER of two lists and the number of pieces is not linear in M;
 * and a control block with the workgroups' counts.  rows == 0 gives a valid handle.  Freeing NULL is SH_OK.  The build
 * runs on the device, once, and is sh_core_graph_create's (one helper serves both), followed by two kernels: the ends of
 * every edge from the run heads of the sorted keys, and the edge id of every list entry by one bisection into them.
 * While it runs the build needs 4 * (rows + 1) + 16 * nnz + 8 bytes for the arrays as given, their flags and scan, 16 bytes
 * per surviving entry for the keys and the sorted keys, 32 bytes per edge for the keys both ways and their sorted copy,
 * and the sort's own scratch; all of it is released before the call returns.  nnz is bounded as for the other handles,
 * and 2M by 2^31 - 256.
 * sh_truss_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 4 * rows + 40 * edges + 51200.
 * sh_truss_graph_edges: M.  sh_truss_graph_max_degree: the largest degree (the length of the longest list).
 *
 * sh_truss: truss: an int32 vector of >= M elements; M = G.edges elements are overwritten, no more.  support, edge_u,
 * edge_v: each NULL, or an int32 vector of >= M elements, of which M are overwritten, no more.  max_rounds >= 0 bounds
 * the rounds; M + 1 can never cut a run short (the Python binding's default); with 0 the call stops after the support
 * pass (support, *triangles and the ends are valid, truss is 0).  M == 0 gives 0 rounds and *complete = 1.  The
 * per-round arrays (capacity max_rounds; each may be NULL) are listed above; ns_per_round is device time, and *total_ns
 * (may be NULL) the device time of the support pass and all rounds (hipEvent) as elsewhere.  A call cut short leaves
 * the handle reusable; g may serve any number of calls, one at a time; every call starts from the support pass.
 * SH_EINVAL: NULL arguments (engine, graph, truss, max_truss, levels, rounds, complete, triangles, out, the arrays),
 * rows < 0, nnz < 0, max_rounds < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases;
 * truss, support, edge_u or edge_v shorter than M.  All are reported before any device work, with the buffers untouched.
 * NOT covered: k-truss subgraph extraction (the edges with truss >= k are one numpy line from truss, edge_u and edge_v),
 * triangle listing, the multi-GPU driver, row pieces (sh_spmv_step_pieces), the C++ harness apps, incremental updates.
 */
typedef struct sh_truss_graph sh_truss_graph;
int sh_truss_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_truss_graph **out);
int sh_truss_graph_free(sh_engine *e, sh_truss_graph *g);
int sh_truss_graph_footprint(const sh_truss_graph *g, uint64_t *device_bytes);
int sh_truss_graph_edges(const sh_truss_graph *g, int64_t *edges);          /* M */
int sh_truss_graph_max_degree(const sh_truss_graph *g, int64_t *entries);
int sh_truss(sh_engine *e, sh_truss_graph *g, sh_vec *truss, sh_vec *support, sh_vec *edge_u, sh_vec *edge_v, int32_t max_rounds,
             int32_t *max_truss, int32_t *levels, int32_t *rounds, int32_t *complete, uint64_t *triangles,
             int32_t *k_per_round, int64_t *size_per_round, int64_t *walked_per_round, uint64_t *ns_per_round,
             uint64_t *total_ns);

/* ---- greedy vertex colouring in a fixed priority order, in Jones-Plassmann rounds -------------------------------------
 * (the reference has no counterpart: its apps are SpMV, PageRank, BFS, SSSP and SCC label propagation; this is the fourth
 * piece on sh_tri's graph, after the triangles, sh_core's core numbers and sh_truss's truss numbers.  A colouring says
 * which rows can be processed together because no entry couples them: the start of a multicolour Gauss-Seidel or SOR
 * sweep, of an incomplete factorisation by colours, of a Jacobian compression, of a lock-free scatter; colour class 0 is
 * a maximal independent set, the start of algebraic-multigrid coarsening.)
 *
 * The graph and the edge rule are sh_tri's, word for word: the matrix is square (rows x rows); entry j of row r storing
 * column c with 0 <= c < rows counts when its 32 value bits are not all zero; the graph is the SIMPLE UNDIRECTED graph
 * under those entries.  Self-loops, parallel entries, stored zeros, the direction of an entry and columns outside the
 * matrix change nothing.  M is its number of edges.
 *      The order.  Vertex v PRECEDES u when (primary(v), tie(v)) > (primary(u), tie(u)), compared lexicographically.
 *      primary(v) is prio[v] (signed int32) when prio is given; otherwise deg[v] when order == 2, else 0.  For order == 0
 *      the tie is "the smaller index first"; for order == 1 and order == 2 it is "the larger mix32(v ^ seed) first", with
 *        mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (on uint32_t).
 *      mix32 is a bijection of the 32-bit words (each step is one), so no two vertices tie and the order is total.  The
 *      three orders are natural first-fit (0), random, JP-R (1) and largest-degree-first, JP-LF (2).  prio makes any other
 *      order reachable: sh_core's core vector as prio approximates smallest-last (no bound on the colours is claimed
 *      for that).
 *      color[v]   = the smallest colour >= 0 held by no neighbour that precedes v: the first-fit colouring that a serial
 *                   loop over the vertices in that order gives (int32, one per vertex).  -1 while v is uncoloured, which
 *                   a caller sees only after a call cut short by max_rounds (*complete is 0 then).
 *      *colors    = the largest colour plus 1 (at most the largest degree plus 1); 0 without rows.
 *      *coloured  = the number of vertices with a colour.
 *      *rounds    = the rounds run; in a complete run the number of vertices on the longest chain v1 precedes v2
 *                   precedes ... along edges.
 *      Round r's list is exactly the vertices whose chain depth is r, so *rounds, size_per_round and edges_per_round (the
 *      sum of the list lengths of the round's vertices) are deterministic.  The colour of a vertex depends only on the
 *      colours of the neighbours that precede it, so a graph and an order have one answer: every comparison is ==.  The
 *      colours do not depend on window, the schedule or the run.
 *
 *      Schedule (csrc/color.hip.h; the work-efficient Jones-Plassmann of Hasenplaugh, Kaler, Schardl, Leiserson, SPAA
 *      2014).  wait[v] is the number of uncoloured neighbours that precede v.  One pass over all lists counts it, the key
 *      of a neighbour computed on the spot (one read of deg[u] or prio[u]; no key array is stored): lists of up to 8
 *      entries one lane, up to 2048 one wave, longer ones in pieces of 2048 with one atomic add per piece.  Behind that
 *      kernel boundary every v with wait[v] == 0 joins the list of round 0.  A round is one fixed set of two launches
 *      enqueued ahead of the host in batches (8, 16, 32, 32, ...), each of which returns at once unless the control block
 *      on the device gives it work.  The first walks the list of every vertex v of the round's work list once: an entry u
 *      with color[u] >= 0 precedes v and its colour is marked as taken; an entry u with color[u] < 0 is preceded by v
 *      and wait[u] gets one atomic decrement -- the one lane that reads the old value 1 owns u and appends it to the next
 *      list.  No key is compared in a round and no restore is needed: each preceding neighbour decrements exactly once.
 *      There is no compare-and-swap, no retry and no waiting.  The marks: one lane keeps a 32-bit mask in a register
 *      (lists of up to 8 entries: the colour is at most 8); one wave a bitmap of 2049 bits in LDS (up to 2048 entries); a
 *      longer list sits at the far end of the work list and a whole workgroup takes it, with an LDS bitmap of `window`
 *      colours (0: 32768 bits, 4 KB) -- when every colour of the window is taken it walks the list again for the next
 *      window, only the first walk decrements, at most len / window + 1 walks.  The second launch sums the workgroups'
 *      counts, folds the largest colour, swaps the lists, records the round and finishes when coloured == rows.  The
 *      work over all rounds is one pass over the lists plus the one for the counts, not one pass per round.
 *      Why that is right: of two neighbours one precedes the other, and the later one's word stays above zero until the
 *      launch that colours the earlier one, so two vertices of one list are never adjacent and no color[u] read in a
 *      launch is written in it.  Every vertex is coloured once and joins a list once, so a list of `rows` places cannot
 *      overflow; no kernel ever waits for another kernel's write; every loop is bounded by a list length, `rows` or
 *      len / window + 1.
 *      Worst cases: the number of rounds is the longest chain in the order, not the diameter -- the natural order on a
 *      path of n vertices takes n rounds, each costing its two launches however small its list is; K_n takes n rounds
 *      under every order, with n walks of n - 1 entries; a long list whose colour lies beyond the first window is walked
 *      once per window up to its colour.
 *
 *      Measured on an MI355X (DESIGN.md "6l Greedy vertex colouring"; tools/color_bench.py, one process per matrix, the
 *        three orders and the host gold alternating, 5 rounds, device time against the wall time of
 *        hostlib.greedy_colors in the same order and process), median (min-max) in ms, rounds, colours: the 2048 x 2048
 *        grid (4 194 304 rows, 8 384 512 edges, largest degree 4): order 0: 63.16 (63.06-63.30), 4095 rounds, 2 colours
 *        (host gold 603); order 1: 3.91 (3.91-3.92), 15, 5 (1259); order 2: 3.93 (3.92-3.93), 15, 5 (1254).  R-MAT-18
 *        (262 144 rows, 3 805 085 edges, largest degree 25 104, degeneracy 374): order 0: 97.74 (97.59-97.77), 943, 162
 *        (281); order 1: 101.73 (101.72-102.15), 916, 168 (317); order 2: 70.20 (70.13-70.26), 883, 123 (311).  R-MAT-20
 *        (1 048 576 rows, 15 702 281 edges, largest degree 64 290, degeneracy 609): order 0: 272.2 (271.9-272.8), 1639,
 *        237 (1266); order 1: 265.1 (265.1-266.1), 1637, 242 (1457); order 2: 161.8 (161.4-162.1), 1506, 182 (1458).
 *        The handle is built in 0.06 s on each.  A round of two launches costs about 15 us however small its list is
 *        (the grid in natural order: 4095 rounds of at most 2048 vertices); on the R-MATs a round costs 79 to 166 us on
 *        average, and the call costs its rounds.
 *        Rule: the binding's default is order = 2, the fewest colours and the fastest arm on both R-MATs and within
 *        0.5 % of order 1 on the grid; a call is 0.003 (grid, orders 1 and 2) to 0.35 (R-MAT-18, order 0) of the host's
 *        serial loop.  Use order 0 only where the natural order is wanted as such: its rounds follow the numbering
 *        (a path numbered end to end takes one round per vertex).  Graphs below 10^6 edges, prio vectors and windows
 *        other than the default are unmeasured.
 *
 * sh_color_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The handle holds on the device:
 * adj_ptr[rows + 1], adj_col[2M] (sh_core_graph's symmetric lists, every list strictly ascending), deg[rows], wait[rows],
 * two work lists of `rows` places each (a vertex joins a list once per call: they cannot overflow), which keep the
 * vertices of the workgroup class at their far end, so that no list of pieces is stored, and a control block with one
 * count per workgroup.  rows == 0 gives a valid handle.  Freeing NULL is SH_OK.  The build runs on the device, once, and
 * is sh_core_graph_create's (one helper serves both): while it runs it needs 4 * (rows + 1) + 16 * nnz + 8 bytes for the
 * arrays as given, their flags and scan, 16 bytes per surviving entry for the keys and the sorted keys, 32 bytes per edge
 * for the keys both ways and their sorted copy, and the sort's own scratch; all of it is released before the call
 * returns.  nnz is bounded as for the other handles, and 2M by 2^31 - 256.
 * sh_color_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 16 * rows + 8 * edges + 17408.
 * sh_color_graph_edges: M.  sh_color_graph_max_degree: the largest degree (the length of the longest list).
 *
 * sh_color: color: an int32 vector of >= rows elements; `rows` elements are overwritten, no more.  prio: NULL, or an
 * int32 vector of >= rows elements, which is only read.  order in 0..2 (the Python binding's default: 2).  seed: any
 * word.  window: 0, or a multiple of 64 in [64, 32768].  max_rounds >= 1 bounds the rounds; rows + 1 can never cut a run
 * short (the Python binding's default).  coloured may be NULL.  The per-round arrays (capacity max_rounds; each may be
 * NULL): size_per_round the vertices of the round's list, edges_per_round the sum of their list lengths, ns_per_round
 * device time.  *total_ns (may be NULL) is the device time of the counting pass and all rounds (hipEvent) as elsewhere.
 * A call cut short leaves the handle reusable; g may serve any number of calls, one at a time; every call starts from
 * the counting pass.  rows == 0 gives SH_OK with zeros and *complete = 1.
 * SH_EINVAL: order outside 0..2, window neither 0 nor a multiple of 64 in [64, 32768], max_rounds < 1 (the scalars are
 * checked first); NULL arguments (engine, graph, color, colors, rounds, complete, out, the arrays), rows < 0, nnz < 0.
 * SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases; color or prio shorter than rows.  All are
 * reported before any device work, with the buffers untouched.
 * NOT covered: distance-2 and bipartite colouring, balancing the classes, recolouring to fewer colours, the
 * smallest-last order as such, the multi-GPU driver, row pieces (sh_spmv_step_pieces), the C++ harness apps, incremental
 * updates.
 */
typedef struct sh_color_graph sh_color_graph;
int sh_color_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_color_graph **out);
int sh_color_graph_free(sh_engine *e, sh_color_graph *g);
int sh_color_graph_footprint(const sh_color_graph *g, uint64_t *device_bytes);
int sh_color_graph_edges(const sh_color_graph *g, int64_t *edges);          /* M */
int sh_color_graph_max_degree(const sh_color_graph *g, int64_t *entries);
int sh_color(sh_engine *e, sh_color_graph *g, sh_vec *color, sh_vec *prio, int32_t order, uint32_t seed, int32_t window,
             int32_t max_rounds, int32_t *colors, int32_t *rounds, int32_t *complete, int64_t *coloured,
             int64_t *size_per_round, int64_t *edges_per_round, uint64_t *ns_per_round, uint64_t *total_ns);

/* ---- minimum spanning forest by Boruvka rounds on an edge list ---------------------------------------------------------
 * (the reference has no counterpart: its apps are SpMV, PageRank, BFS, SSSP and SCC label propagation.  sh_wcc, sh_tri,
 * sh_core, sh_truss and sh_color read only the pattern; sh_sssp reads the weights but is directed and has a source.  This
 * is the first weighted undirected entry point: which edges of a symmetric matrix of distances, conductances or
 * similarities form the cheapest skeleton that keeps everything connected.)
 *
 * The graph.  The graph rule is sh_truss's, unchanged: the matrix is square (rows x rows); entry j of row r storing
 * column c with 0 <= c < rows counts when its 32 value bits are not all zero; the graph is the SIMPLE UNDIRECTED graph
 * under those entries.  Self-loops, stored zeros and columns outside the matrix change nothing.  Edge e, 0 <= e < M, is the
 * e-th smallest pair u < v.
 *      Weights.  The values are float32.  Weights are compared by the total order of their bit patterns: with b the bits,
 *      k(b) = b ^ 0xFFFFFFFF if the sign bit is set, else b ^ 0x80000000.  This gives the order -NaN < -inf < ... < -0.0 <
 *      denormals < ... < +inf < +NaN.  Nothing is refused: NaN and infinities are legal weights with a defined place.  A
 *      stored +0.0 is no edge, by the graph rule.  The weight of edge {u, v} is the smallest, by k, over all counting
 *      entries (u, v) and (v, u), parallel entries included: an unsymmetric or duplicated matrix has one answer.
 *      KEY(e) = k(weight[e]) << 32 | e.  No two keys are equal.
 *      The result is the unique minimum spanning forest under KEY: what Kruskal's algorithm returns when it takes the
 *      edges in ascending KEY.
 *      in_msf[e]   = 1 or 0 (int32).  M elements are overwritten, no more.
 *      comp[v]     = the largest vertex index of v's component (optional; the convention of sh_wcc and sh_scc: it equals
 *                    sh_wcc's comp on the same arrays).
 *      edge_u, edge_v (optional): as in sh_truss.  weight[e] (optional): the 32 bits of the chosen entry.
 *      *tree_edges = rows - *components.  *components = the number of v with comp[v] == v.
 *      Every comparison is ==.  The result does not depend on the schedule or the run.
 *
 *      Schedule (csrc/msf.hip.h; Boruvka 1926 on a parent forest, as Vineet, Harish, Patidar and Narayanan did on a GPU in
 *      2009).  There is no compare-and-swap, no retry, and no lane waits for another.  State on the device: p[v] the
 *      parent word, best[v] one 64-bit word per vertex, to[v] the root that a root will hook to, eu[M], ev[M], wk[M] the
 *      ends and k(weight) of every edge, two work lists of M edge ids.  The work item is an edge of a flat list: there are
 *      no long rows and no pieces, every lane gets one edge.  At the start of every round every tree is a star: p[v] is a
 *      root for all v.  Round 1 has p[v] = v and the list holds all M edges.  A round is one fixed set of launches
 *      enqueued ahead of the host in batches (8, 16, 32, 32, ...), each of which returns at once unless the control block
 *      on the device gives it work.
 *      find: best[.] = MAX was written by a launch that ended before this one.  For every edge e of the list, a = p[eu[e]]
 *      and b = p[ev[e]].  If a == b the edge is inside a tree for good and is dropped.  Otherwise it is appended to the
 *      next list with a wave-aggregated push -- such an edge enters a list once per round, so M places cannot overflow --
 *      and KEY(e) goes into best[a] and best[b] with one 64-bit atomic minimum each (one global_atomic_umin_x2).  The
 *      atomic is issued only if KEY(e) is below a load of the word: the word only falls, so a stale read can only let a
 *      needless atomic through and never suppresses a needed one.
 *      pick: every root r with best[r] != MAX takes e = the low 32 bits and stores in_msf[e] = 1 (two roots that chose the
 *      same edge store the same value), finds the other root o among p[eu[e]] and p[ev[e]] and writes to[r] = o.  The one
 *      exception is a mutual pair with r > o: when best[o] == best[r], the smaller index hooks and the larger stays a
 *      root.  pick reads p and writes only to and in_msf: the launch that decides the hooks must not read a word that the
 *      same launch writes.
 *      link: p[r] = to[r]; the lane puts best[r] back to MAX (nobody else looks at the word in that launch).
 *      jump: each of MSF_SWEEPS = 8 launches runs over all vertices, with at most MSF_JUMPS = 16 stores of
 *      p[v] = p[p[v]] per vertex; sweep i > 0 returns at once unless sweep i - 1 moved a pointer.  The bound holds for any
 *      order of the lanes: a lane that runs before the vertices above it sees old pointers and gains only one hop per
 *      jump, so a launch shortens a depth d to at most ceil(d / (MSF_JUMPS + 1)), not to d / 2^MSF_JUMPS.
 *      (MSF_JUMPS + 1)^MSF_SWEEPS = 17^8 >= 2^31 (a static_assert): every tree is a star again when the round ends, on any
 *      input and any schedule.
 *      close: sums the workgroups' counts, records the round, swaps the lists.  It finishes when find kept no edge; in
 *      that round pick, link and the jumps return at once.
 *      After the last round top[root] = max v by one atomic maximum per vertex at most (top lives in best's memory; the
 *      vertices are taken from the largest down and a lane sends nothing when the word is already at or above its
 *      index), comp[v] = top[p[v]], and the roots are counted.
 *      Why that is right: all keys differ, so the lightest edge leaving a tree is in the one minimum spanning forest (the
 *      cut property), whatever the other trees do in that round.  In the graph "root -> chosen other root" every cycle
 *      has length 2: along a cycle the chosen keys would have to fall strictly unless both ends chose one edge; the
 *      mutual rule breaks exactly those cycles, so link builds a forest.  Pointers never leave a component.  A run ends
 *      when no listed edge joins two trees; dropped edges were inside a tree and trees only merge, so every component is
 *      one star.
 *      Determinism: find sees one state, so the set of kept edges, best, the hooks, *rounds, walked_per_round (the list
 *      length at the start), kept_per_round and hooks_per_round (to pointers applied) are functions of the input alone.
 *      Only the order inside a list, jumps_per_round and the times may differ from run to run.
 *      Rounds: every tree with a leaving edge merges, so a run has at most floor(log2(rows)) + 1 rounds, the empty last
 *      one included.  The Python default max_rounds = 33 can never cut a run short.  After a run cut short
 *      (*complete == 0) in_msf holds the tree edges found so far, every one of which belongs to the forest, *components
 *      is the number of trees so far and *tree_edges = rows - *components the edges found so far; comp is -1 everywhere
 *      and the handle is good for another call.
 *      Worst cases: the work is the sum of the list lengths, M log(rows) at worst; an edge inside a tree is walked once
 *      more before it goes.  Late rounds send every edge on the rim of the giant tree to one best word: the pre-check
 *      keeps the atomics to the falling prefix minima, but the loads still meet on one line.  Every round costs its
 *      launches (12, of which up to 11 return at once) however short its list is.
 *
 *      Measured on an MI355X (DESIGN.md "6m Minimum spanning forest"; tools/msf_bench.py, one process per matrix, sh_msf,
 *        the host gold and sh_wcc alternating, 5 rounds, device time against the wall time of hostlib.msf_edges in the
 *        same process; drawn weights: one float32 in [0, 1) per stored entry), median (min-max) in ms, rounds: the 2048 x
 *        2048 grid (4 194 304 rows, 8 384 512 edges): drawn weights 6.71 (6.69-6.72), 13 rounds, 29.0 M edges walked (host
 *        gold 1549); unit weights 1.88 (1.88-1.92), 2 rounds -- one round hooks 4 194 303 roots into chains that the sweeps
 *        flatten with 74.6 M pointer stores -- (host gold 680).  R-MAT-18 (262 144 rows, 3 805 085 edges, 88 129
 *        components), drawn weights: 3.88 (3.79-4.88), 5 rounds, 17.5 M edges walked (host gold 510); its rounds cost 778,
 *        761, 780 and 698 us for lists of 3.81, 3.81, 3.64 and 3.54 M edges.  A star of 70 001 leaves (one best word
 *        wanted by every edge): 0.36 (0.31-0.40), its merging round 298 us, the empty round behind it 25 us (host gold
 *        3.87).  sh_wcc on the same arrays: 0.39, 0.38, 0.33 and 0.88 ms.  The handle is built in 0.05 to 0.07 s.
 *        Rule: a call is 0.003 to 0.008 of the host's Kruskal on graphs of 4 to 8 million edges and 0.09 of it on the
 *        star; the device lost on none of the inputs measured.  A round costs at least its twelve launches (25 us), so on
 *        graphs of a few thousand edges the host is expected to win; where exactly, R-MAT-18 with unit weights and graphs
 *        above 10^7 edges are unmeasured.  For the components alone call sh_wcc.
 *
 * sh_msf_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The handle holds on the device:
 * p[rows], to[rows], best[rows] (64-bit), eu[M], ev[M], wk[M], two work lists of M places each and a control block with
 * two counts per workgroup; no adjacency lists.  rows == 0 gives a valid handle.  Freeing NULL is SH_OK.  The build runs
 * on the device, once: the first half of sh_truss_graph_create's (the entries that count as sorted keys, the first of
 * every run an edge), the ends of every edge, and one pass over the nnz entries as given that applies the edge rule
 * again, bisects (min, max) into eu / ev and takes the atomic minimum of k(val) into wk[e].  While it runs it needs
 * 4 * (rows + 1) + 16 * nnz + 8 bytes for the arrays as given, their flags and scan, 4 * rows for the degrees the shared
 * builder counts, 16 bytes per surviving entry for the keys and the sorted keys, and the sort's own scratch; all of it is
 * released before the call returns.  nnz is bounded as for the other handles, and 2M <= 2^31 - 256.
 * sh_msf_graph_footprint: device bytes held =
 *     16 * rows + 20 * edges + 33792.
 * sh_msf_graph_edges: M.
 *
 * sh_msf: in_msf: an int32 vector of >= M elements.  comp: NULL, or an int32 vector of >= rows elements.  edge_u, edge_v,
 * weight: NULL, or vectors of >= M elements each.  max_rounds >= 1 bounds the rounds.  The per-round arrays (capacity
 * max_rounds; each may be NULL): walked_per_round, kept_per_round, hooks_per_round, jumps_per_round (pointers changed by
 * the sweeps), ns_per_round device time.  *total_ns (may be NULL) is the device time of the start, all rounds and the
 * labels (hipEvent) as elsewhere.  One handle serves any number of calls, one at a time.  rows == 0 gives SH_OK with
 * zeros and *complete = 1.
 * SH_EINVAL: max_rounds < 1 (the scalars are checked first); NULL arguments (engine, graph, in_msf, tree_edges,
 * components, rounds, complete, out, the arrays), rows < 0, nnz < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or
 * a row_ptr that decreases; in_msf, edge_u, edge_v or weight shorter than M, comp shorter than rows.  All are reported
 * before any device work, with the buffers untouched.
 * NOT covered: the total weight (one numpy line: weight[in_msf == 1].astype(float64).sum() on the float32 view), maximum
 * spanning forests (negate the values), a tree as parent pointers from a chosen root, the multi-GPU driver, row pieces
 * (sh_spmv_step_pieces), the C++ harness apps, incremental updates.
 */
typedef struct sh_msf_graph sh_msf_graph;
int sh_msf_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_msf_graph **out);
int sh_msf_graph_free(sh_engine *e, sh_msf_graph *g);
int sh_msf_graph_footprint(const sh_msf_graph *g, uint64_t *device_bytes);
int sh_msf_graph_edges(const sh_msf_graph *g, int64_t *edges);            /* M */
int sh_msf(sh_engine *e, sh_msf_graph *g, sh_vec *in_msf, sh_vec *comp, sh_vec *edge_u, sh_vec *edge_v, sh_vec *weight,
           int32_t max_rounds, int64_t *tree_edges, int64_t *components, int32_t *rounds, int32_t *complete,
           int64_t *walked_per_round, int64_t *kept_per_round, int64_t *hooks_per_round, int64_t *jumps_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns);

/* ---- greedy weighted matching by rounds of locally dominant edges on an edge list -------------------------------------
 * (the reference has no counterpart.  sh_msf answers "which edges form the cheapest skeleton" of a symmetric matrix;
 * this answers the question asked next: which unknowns are coupled most strongly and should be merged in pairs when the
 * matrix is coarsened -- pairwise aggregation in algebraic multigrid, heavy-edge coarsening in partitioners, pairing
 * pivots.  Class 0 of sh_color is an independent set of vertices, not of edges.)
 *
 * The graph and the edge weights are sh_msf's, unchanged: the matrix is square; entry j of row r storing column c with
 * 0 <= c < rows counts when its 32 value bits are not all zero; the graph is the SIMPLE UNDIRECTED graph under those
 * entries.  Self-loops, stored zeros and columns outside the matrix change nothing.  Edge e, 0 <= e < M, is the e-th
 * smallest pair u < v.  Weights are float32 compared by k(b) = b ^ 0xFFFFFFFF if the sign bit is set, else
 * b ^ 0x80000000; the weight of edge {u, v} is the smallest, by k, over all counting entries (u, v) and (v, u), parallel
 * entries included.  NaN and infinities have their place in the order.  Nothing is refused.  A stored +0.0 is no edge.
 *      The order of a call.  Two scalars fix it: heavy is 0 or 1, seed any uint32.
 *        MKEY(e) = hi(e) << 32 | lo(e)
 *        hi = k(weight[e]) for heavy == 0 (lightest first), hi = ~k(weight[e]) for heavy == 1 (heaviest first: the
 *        Python default, what coarsening wants);
 *        lo = e when seed == 0, lo = mix32(e ^ seed) otherwise, mix32 being sh_color's bijection of the 32-bit words.
 *      Both forms of lo are bijections of e, so no two keys are equal, and the result is unique: the greedy matching,
 *      what a serial loop returns when it takes the edges in ascending MKEY and keeps an edge when both its ends are
 *      still free.  It is maximal, and under heavy == 1 with non-negative weights its weight is at least half the
 *      maximum weight of a matching (the 1/2-approximation of Avis 1983).  A key may be all ones only for seed != 0 (for
 *      seed == 0, e < 2^31), on the one edge with mix32(e ^ seed) == 0xFFFFFFFF when its weight is the last of the
 *      order; that is harmless (csrc/match.hip.h says why) and nothing is masked.
 *      mate[v]     = the partner of v, or -1 (int32).  rows elements are overwritten, no more.
 *      in_match[e] = 1 or 0 (int32; optional).  M elements are overwritten, no more.
 *      edge_u, edge_v, weight (optional): as in sh_msf.
 *      *pairs      = the number of matched edges = the number of v with mate[v] > v.
 *      Every comparison is ==.  The result does not depend on the schedule or the run.
 *
 *      Schedule (csrc/match.hip.h; the locally dominant edges of Preis 1999, Hoepman 2004 and Manne and Bisseling 2007).
 *      There is no compare-and-swap, no retry, and no lane waits for another.  State on the device: best[v] one 64-bit
 *      word per vertex, eu[M], ev[M], wk[M] the ends and k(weight) of every edge, two work lists of M edge ids; mate is
 *      the caller's vector.  The work item is an edge of a flat list, one lane per edge.  A round is one fixed set of
 *      four launches enqueued ahead of the host in batches (8, 16, 32, 32, ...), each of which returns at once unless the
 *      control block on the device gives it work.  Round r walks its list; walked_r is the list's length.
 *      bid: best[.] = MAX for every free vertex with a listed edge was written by an earlier launch.  An edge with a
 *      matched end is dropped for good.  Every other edge is kept: it is appended to the next list with a wave-aggregated
 *      push -- an edge enters a list once per round, so M places cannot overflow -- and MKEY(e) goes into best[eu[e]] and
 *      best[ev[e]] with the pre-checked 64-bit atomic minimum of sh_msf (one global_atomic_umin_x2).  kept_r edges go on.
 *      take: walks the next list.  Edge e is matched when best[eu[e]] == MKEY(e) && best[ev[e]] == MKEY(e): it is the
 *      smallest key among the kept edges at both its ends (locally dominant).  The edge tests itself, so nothing inverts
 *      mix32.  It stores mate[eu] = ev, mate[ev] = eu and in_match[e] = 1; two matched edges share no end.  take reads
 *      best and writes mate, bid reads mate and writes best: neither launch reads what it writes itself.  matched_r
 *      edges are matched.
 *      clear: best = MAX at both ends of every kept edge (concurrent stores store the same value).  A vertex whose edges
 *      were all dropped is never bid for again.
 *      close: one workgroup sums the workgroups' counts, records the round and swaps the lists.  The run ends at the first
 *      round with kept_r == 0; that round is counted, and take and clear return at once in it.
 *      Why that is right, by induction over the rounds.  Suppose an edge (u, w) died at u before (u, v) was dominant.  It
 *      died because w was matched through some (w, x).  That edge was dominant while (u, w) was still kept, so its key is
 *      smaller: greedy reached (w, x) first and, by induction, took it.  So greedy never takes (u, w), every edge at u or
 *      v with a key below MKEY(u, v) is of that kind, and both u and v are free when greedy reaches (u, v): greedy takes
 *      it.  A dropped edge has a matched end, so greedy does not take it.
 *      Determinism: bid sees one state, so *rounds, walked_per_round, kept_per_round, matched_per_round, mate and
 *      in_match are functions of the input, heavy and seed alone.  Only the order inside a list and the times may differ
 *      from run to run.
 *      Rounds: every round with kept_r > 0 matches at least one edge (the smallest kept key of all is dominant), and a
 *      pair takes two vertices, so rounds <= floor(rows / 2) + 1.  The bound is attained on a path whose keys ascend
 *      along it.  The Python default max_rounds = 4096 is a cap on the device time, not a bound.  After a run cut short
 *      (*complete == 0) mate and in_match hold the pairs found so far, every one of which belongs to the greedy
 *      matching: a valid matching, not a maximal one.  The handle is good for another call.
 *      Worst cases: a path, or any graph, with equal weights and seed == 0 has keys that ascend with the edge id and gets
 *      one pair per round in places; that is what seed is for, and why the Python default is seed = 1.  A hub sends every
 *      kept edge to one best word: the pre-check keeps the atomics to the falling prefix minima, but the loads meet on
 *      one line.  Every round costs its four launches however short its list is.
 *
 *      Measured on an MI355X (DESIGN.md "6n Greedy matching"; tools/match_bench.py, one process per matrix, sh_match
 *        under heavy 0 / 1 and seed 0 / 1 and the host gold alternating, 5 rounds, device time against the wall time of
 *        hostlib.greedy_matching in the same process; drawn weights: one float32 in [0, 1) per stored entry), median
 *        (min-max) in ms for heavy = 1, seed = 1:
 *        the 2048 x 2048 grid (4 194 304 rows, 8 384 512 edges), drawn weights: 3.75 (3.74-3.75), 8 rounds, 18.8 M edges
 *        walked, 1 901 973 pairs (host gold 1229); its rounds cost 1622, 1576, 350, 80, 23, 16, 14 and 13 us for lists of
 *        8.38, 8.38, 1.69 and 0.30 M edges and less.  The same grid with unit weights: 3.75 (3.75-3.75), 8 rounds, 18.8 M
 *        edges walked, 1 901 716 pairs (host gold 1184); with seed = 0, measured once: 4165 ms, 3072 rounds, 12 884 M edges
 *        walked, 2 097 152 pairs (host gold 690) -- 6.0 times the host, and the reason for the default seed.  R-MAT-18
 *        (262 144 rows, 3 805 085 edges), drawn weights: 1.71 (1.68-1.75), 11 rounds, 8.8 M edges walked, 39 623 pairs
 *        (host gold 486).  A star of 70 001 leaves (one best word wanted by every edge): 0.34 (0.33-0.38), 2 rounds, its
 *        matching round 312 us, the empty round behind it 13 us (host gold 3.68).  heavy = 0 and, on drawn weights,
 *        seed = 0 cost the same within 5 % (profiles/match_*.json).  The handle is built in 0.05 to 0.06 s.
 *        Rule: with seed != 0, or with weights that differ, a call is 0.003 to 0.004 of the host's sort-and-take loop on
 *        graphs of 4 to 8 million edges and 0.09 of it on the star; the device lost on none of those.  With equal weights
 *        and seed = 0 it lost by a factor of 6 on the grid: do not call it that way.  A round costs at least its four
 *        launches (13 us), so on graphs of a few hundred edges the host is expected to win; where exactly, R-MAT-18 with
 *        unit weights and graphs above 10^7 edges are unmeasured.
 *
 * sh_match_graph_create: the handle is made from the host CSR arrays alone (no sh_csr), by the builder of
 * sh_msf_graph_create (the same temporaries and bounds: 2M <= 2^31 - 256).  The handle holds on the device: best[rows]
 * (64-bit), eu[M], ev[M], wk[M], two work lists of M places each and a control block with one count per workgroup; no
 * adjacency lists.  rows == 0 gives a valid handle.  Freeing NULL is SH_OK.
 * sh_match_graph_footprint: device bytes held =
 *     8 * rows + 20 * edges + 17408.
 * sh_match_graph_edges: M.
 *
 * sh_match: mate: an int32 vector of >= rows elements.  in_match, edge_u, edge_v, weight: NULL, or vectors of >= M
 * elements each.  heavy: 0 or 1.  seed: any.  max_rounds >= 1 bounds the rounds.  The per-round arrays (capacity
 * max_rounds; each may be NULL): walked_per_round, kept_per_round, matched_per_round, ns_per_round device time.
 * *total_ns (may be NULL) is the device time of the start and all rounds (hipEvent) as elsewhere.  One handle serves any
 * number of calls, one at a time; heavy and seed may differ from call to call.  rows == 0 gives SH_OK with zeros and
 * *complete = 1.
 * SH_EINVAL: max_rounds < 1, heavy outside {0, 1} (the scalars are checked first); NULL arguments (engine, graph, mate,
 * pairs, rounds, complete, out, the arrays), rows < 0, nnz < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a
 * row_ptr that decreases; mate shorter than rows; in_match, edge_u, edge_v or weight shorter than M.  All are reported
 * before any device work, with the buffers untouched.
 * NOT covered: maximum-cardinality or maximum-weight matching (this is the greedy 1/2-approximation), bipartite
 * row-column matching (the graph here is the symmetric one on the rows), the aggregate map of a coarsening (one numpy
 * line: np.minimum(v, mate) where mate >= 0, else v), continuing a cut-short run (a new call starts over), the multi-GPU
 * driver, the C++ harness apps.
 */
typedef struct sh_match_graph sh_match_graph;
int sh_match_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_match_graph **out);
int sh_match_graph_free(sh_engine *e, sh_match_graph *g);
int sh_match_graph_footprint(const sh_match_graph *g, uint64_t *device_bytes);
int sh_match_graph_edges(const sh_match_graph *g, int64_t *edges);          /* M */
int sh_match(sh_engine *e, sh_match_graph *g, sh_vec *mate, sh_vec *in_match, sh_vec *edge_u, sh_vec *edge_v, sh_vec *weight,
             int32_t heavy, uint32_t seed, int32_t max_rounds, int64_t *pairs, int32_t *rounds, int32_t *complete,
             int64_t *walked_per_round, int64_t *kept_per_round, int64_t *matched_per_round, uint64_t *ns_per_round,
             uint64_t *total_ns);

/* ---- reverse Cuthill-McKee ordering in level-synchronous steps ----------------------------------------------------------
 * (the reference has no counterpart.  After sh_color, sh_msf and sh_match this is the fourth question a user asks of a
 * sparse matrix before solving with it: how to renumber it so that its entries stand near the diagonal -- a smaller
 * bandwidth and profile for a banded or skyline factorisation, and columns that stay close for the x gather of SpMV.)
 *
 * The graph is sh_core's and sh_color's: the matrix is square (rows x rows); entry j of row r storing column c with
 * 0 <= c < rows counts when its 32 value bits are not all zero; the graph is the SIMPLE UNDIRECTED graph under those
 * entries.  Self-loops, parallel entries, stored zeros, the direction of an entry and columns outside the matrix change
 * nothing.  deg[v] is the degree; "smaller" means the smaller pair (deg, index).
 *      The definition (a serial loop; host/src/rcm_order.cpp is it, word for word).  Walk the vertices in ascending
 *      (deg, index).  For every vertex v without a position yet:
 *        1. The root, by George and Liu with a cap.  r = v.  With sweeps == 0 that is all.  Otherwise a breadth-first
 *           search from r gives its eccentricity e and its last level; then at most `sweeps` times: x = the smallest
 *           vertex of the last level; if x == r stop; the search from x gives e'; if e' > e take r = x, e = e' and that
 *           search's last level and go on, otherwise stop and keep r.
 *        2. Cuthill-McKee from r: r takes the next position; the vertices are then taken in position order, and each
 *           one's neighbours without a position are appended in ascending (deg, index).
 *      With reverse == 1 position k becomes rows - 1 - k.
 *      perm[k]   = the vertex at new position k (int32; scipy's convention: A[perm][:, perm] is the reordered matrix).
 *      pos[v]    = the new position of v, the inverse of perm (int32; optional).
 *      level[v]  = the level of v in the search from its component's final root (int32; optional).
 *      Vertices without an edge come first in the walk; each is its own component and takes no step.
 *      *components = the components numbered.  *sweeps_run = the searches run to find roots (the one from v included).
 *      *bandwidth_before / _after = max |p(u) - p(v)| over the edges, *profile_before / _after = the sum over v of
 *      p(v) - min(p(v), min over the neighbours u of p(u)), p being the identity and the new position; exact, 64-bit.
 *      A STEP is one level of one search: a search of eccentricity e takes e + 1 steps, and its last step finds nothing.
 *      kind_per_step is 0 for a level of a root search and 1 for a level of the numbering, size_per_step the level's
 *      width, edges_per_step the sum of its list lengths.  A run takes at most (sweeps + 2) * rows steps.  With the
 *      ties fixed as above the answer is unique: every comparison is ==, the records included.
 *
 *      Schedule (csrc/rcm.hip.h).  The handle sorts the vertices once by deg << 32 | index and builds the symmetric lists
 *      over those LABELS, so the smaller (deg, index) is the smaller label and every list stands in child order.  The
 *      numbering runs level by level: the level occupies positions [a, b) of the order array; a vertex w of the next
 *      level belongs to the smallest position of [a, b) adjacent to it (atomicMin(owner[w], i)); every position counts
 *      the entries of its list that it owns; a prefix sum over the counts -- per workgroup over a contiguous chunk, the
 *      workgroups' totals scanned by each -- gives position i's children their places b + offset + k in list order.  That
 *      is the serial order: the serial loop appends w when it reaches the first position that has w in its list.  The
 *      order array is its own queue and nothing is sorted per level.  A level of a root search is unordered: a stamp per
 *      vertex holds the generation of the search that reached it (generations count down, so claiming is an atomic
 *      minimum and nothing is cleared between searches), the queue is the free part of the order array, and the smallest
 *      label of the new level is an atomic minimum.  A step is one fixed set of five launches enqueued ahead of the host
 *      in batches (8, 16, 32, 32, ...), each of which returns at once unless the control block gives it work; the last is
 *      one workgroup that records the step and chooses the next: the next level, a search from x, the numbering from r,
 *      the next component (a cursor over the labels) or the end.  Lists of up to 8 entries are walked by a lane, up to
 *      2048 by a wave (ranked by a ballot prefix), longer ones by the workgroup in chunks of 256.  Every exchange between
 *      workgroups crosses a launch boundary; there is no compare-and-swap, no spin and no flag.
 *      Worst cases: a step costs its five launches however narrow its level is, so a long thin graph (a path, a grid:
 *      4095 levels per search on 2048 x 2048) pays per level, and a matrix with thousands of small components pays several
 *      steps for each.
 *
 *      Measured on an MI355X (DESIGN.md "6o Reverse Cuthill-McKee"; tools/rcm_bench.py, one process per matrix, sweeps
 *        0 / 2 / 8 and the host gold alternating, 5 rounds, device time against the wall time of hostlib.rcm_order in the
 *        same process), median (min-max) in ms for sweeps = 8: the 2048 x 2048 grid (4 194 304 rows, 8 384 512 edges):
 *        280.5 (267.7-282.7), 12 285 steps, 2 searches, bandwidth 2048 -> 2048 (host gold 1135); the same grid with its
 *        vertices shuffled: 338.5 (308.7-341.8), bandwidth 4 191 905 -> 2048 (2733); R-MAT-18 (262 144 rows, 3 805 085
 *        edges): 18.54 (18.02-18.71), 338 steps, 103 searches, 146 419 (581); synth:scircuit (170 998 rows, 958 718
 *        edges): 3.63 (3.59-3.65), 35 steps, 131 287 (121).  sweeps = 0 costs 111.6, 127.2, 7.24 and 0.90 ms.  A step
 *        costs 19 to 29 us on the grid however narrow its level is.  The handle is built in 0.05 to 0.06 s.  sh_spmv on
 *        A[perm][:, perm] against A, both under the default plan, us per call: 47.2 against 52.6 on the grid, 47.3
 *        against 58.1 on the shuffled grid, 25.1 against 31.3 on R-MAT-18, 12.9 against 13.5 on synth:scircuit.
 *        Rule: a call is 0.03 of the host's serial loop on the two power-law matrices and 0.12 to 0.25 of it on the
 *        grids; the device lost on none of the four.  Graphs below 10^5 rows, matrices with thousands of small
 *        components that have edges, and matrices whose x does not fit in L2 are unmeasured.
 *
 * sh_rcm_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  The handle holds on the device:
 * adj_ptr[rows + 1], adj_col[2M] (the symmetric lists over the labels, every list strictly ascending), S[rows] (label ->
 * vertex), order, posl, levl, stamp, owner and cnt (`rows` words each) and a control block with a count per workgroup.
 * rows == 0 gives a valid handle.  Freeing NULL is SH_OK.  The build runs on the device, once: while it runs it needs
 * what sh_core_graph_create needs and 24 bytes per row for the degrees, the sort keys and the inverse of S; all of it is
 * released before the call returns.  nnz is bounded as for the other handles, and 2M by 2^31 - 256.
 * sh_rcm_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 28 * rows + 8 * edges + 50176.
 * sh_rcm_graph_edges: M.  sh_rcm_graph_max_degree: the largest degree (the length of the longest list).
 *
 * sh_rcm: perm: an int32 vector of >= rows elements; pos, level: NULL, or such vectors; `rows` elements of each are
 * overwritten, no more.  sweeps in [0, 64] (the Python binding's default: 8).  reverse: 0 or 1 (default 1).
 * max_steps >= 1 bounds the steps; (sweeps + 2) * rows + 1 can never cut a run short.  The per-step arrays (capacity
 * max_steps; each may be NULL): kind_per_step, size_per_step, edges_per_step, ns_per_step device time.  *total_ns (may be
 * NULL) is the device time of the start, all steps and the closing launch (hipEvent) as elsewhere.  A run cut short
 * returns *complete = 0: the numbered part of perm is as the full run would give it, the rest of perm is -1, pos and
 * level of the vertices without a position are -1, and *bandwidth_after and *profile_after are -1.  The handle is good
 * for another call; one handle serves any number of calls, one at a time.  rows == 0 gives SH_OK with zeros and
 * *complete = 1.
 * SH_EINVAL: sweeps outside [0, 64], reverse outside {0, 1}, max_steps < 1 (the scalars are checked first); NULL arguments
 * (engine, graph, perm, components, sweeps_run, steps, complete, the bandwidths and profiles, out, the arrays), rows < 0,
 * nnz < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases; perm, pos or level shorter than
 * rows.  All are reported before any device work, with the buffers untouched.
 * NOT covered: orderings other than RCM (Sloan, nested dissection, minimum degree), running small components
 * concurrently, permuting an uploaded sh_csr on the device, the multi-GPU driver, the C++ harness apps.
 */
typedef struct sh_rcm_graph sh_rcm_graph;
int sh_rcm_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_rcm_graph **out);
int sh_rcm_graph_free(sh_engine *e, sh_rcm_graph *g);
int sh_rcm_graph_footprint(const sh_rcm_graph *g, uint64_t *device_bytes);
int sh_rcm_graph_edges(const sh_rcm_graph *g, int64_t *edges);          /* M */
int sh_rcm_graph_max_degree(const sh_rcm_graph *g, int64_t *entries);
int sh_rcm(sh_engine *e, sh_rcm_graph *g, sh_vec *perm, sh_vec *pos, sh_vec *level, int32_t sweeps, int32_t reverse,
           int32_t max_steps, int32_t *components, int32_t *sweeps_run, int32_t *steps, int32_t *complete,
           int64_t *bandwidth_before, int64_t *bandwidth_after, int64_t *profile_before, int64_t *profile_after,
           int32_t *kind_per_step, int64_t *size_per_step, int64_t *edges_per_step, uint64_t *ns_per_step,
           uint64_t *total_ns);

/* ---- betweenness centrality by Brandes' two sweeps, in float64 -------------------------------------------------------------
 * (the reference has no counterpart.  Of the six kernels a graph library is measured by -- BFS, SSSP, PageRank, connected
 * components, triangle counting, betweenness centrality -- this is the last one: which vertices the shortest paths run
 * through.  Brandes, "A faster algorithm for betweenness centrality", J. Math. Sociol. 2001.)
 *
 * The edge rule is sh_bfs_levels's: the matrix is square (rows x rows); an edge c -> r exists when row r stores column c
 * with 0 <= c < rows and a value whose 32 bits are not all zero.  The graph is the SIMPLE DIRECTED graph under those
 * entries: parallel entries are one edge and self-loops are none (a shortest-path count must not see a stored duplicate
 * as a second path); stored zeros and columns outside the matrix are legal and are no edges.
 *      For a source s:
 *      level_s(v) = the BFS distance from s, -1 if unreached.
 *      sigma_s(v) = the number of shortest s -> v paths: sigma_s(s) = 1, 0 if v is unreached, else the sum over the
 *                   edges u -> v with level(u) == level(v) - 1 of sigma_s(u).
 *      delta_s(v) = the sum over the edges v -> w with level(w) == level(v) + 1 of (sigma(v) / sigma(w)) * (1 + delta(w)).
 *      bc[v]      = the sum over the sources, in the order given, of delta_s(v) for v != s.
 *      Endpoints are not counted and nothing is normalised: on a symmetric pattern every unordered pair counts twice, and
 *      halving is the caller's line.  A source may occur twice and then counts twice.
 *
 *      Arithmetic.  sigma, delta and bc are IEEE float64.  sigma is exact while it stays below 2^53, rounded above, and
 *      +inf above the float64 range, after which that source's delta is whatever IEEE gives (inf / inf is a NaN, whose
 *      sign and payload IEEE leaves open).  Nothing is refused: sigma_max_per_source returns the largest sigma of every
 *      source, so the caller sees which case holds.  THE ORDER OF EVERY ADDITION IS PART OF THE RESULT, and it is fixed
 *      here, once, as a function of the list alone -- its entries in ascending neighbour index and its length:
 *        SUM(list): entry j of the list contributes the term t[j], +0.0 where the entry does not take part (a neighbour
 *        on another level).  The list is cut into pieces of 2048 entries, the last one shorter.  Inside a piece there are
 *        64 strided partials, partial[l] = (((+0.0 + t[l]) + t[l + 64]) + t[l + 128]) + ..., folded by a fixed butterfly:
 *        for o = 32, 16, 8, 4, 2, 1: partial[l] = partial[l] + partial[l ^ o] for all l at once; the piece's sum is
 *        partial[0].  The piece sums are added left to right, starting from +0.0.  The empty list sums to +0.0.
 *      Every term is non-negative, so padding with +0.0 is exact, and a list of up to 8 entries sums to
 *      ((t0 + t4) + (t2 + t6)) + ((t1 + t5) + (t3 + t7)).  sigma_s(v) = SUM over v's in-list, delta_s(v) = SUM over v's
 *      out-list with the term (sigma(v) / sigma(w)) * (1 + delta(w)) -- one correctly rounded division, one addition, one
 *      multiplication, no fused multiply-add --, and bc[v] = bc[v] + delta_s(v), source after source, for the vertices v
 *      of the levels 1 .. depth - 1 (the others have delta +0.0 or are the source).  With that every comparison is ==:
 *      tests/bc_ref.py restates SUM in numpy and host/src/bc_scores.cpp in C++.
 *
 *      Why the result is schedule-free: one owner per value.  sigma[w] is computed by the one lane or wave that pulls
 *      over w's in-list, delta[v] and bc[v] by the one that pulls over v's out-list, from values that launches which
 *      ended before have written.  There are no float atomics.  The queue order decides who computes a value, never from
 *      what or in which order, so no value depends on the queue order, the grid, the batch size or the run; the same
 *      SUM serves a lane (up to 8 entries), a wave (up to a piece) and a wave over several pieces.
 *
 *      Schedule (csrc/bc.hip.h).  The handle holds the surviving entries as 64-bit keys, sorted and deduplicated as
 *      sh_tri_graph_create does, as in-lists and out-lists, both strictly ascending; per vertex a level word, sigma and
 *      delta; one order array that is its own queue, with the start of every level kept on the device.  Forward, one step
 *      per level, enqueued ahead of the host in batches (8, 16, 32, 32, ...) of gated launches: bc_expand pushes the
 *      out-lists of the level (atomicMin on the unsigned level word claims w, and the one lane that saw it unreached
 *      appends it: no compare-and-swap; out-lists above 2048 entries are pushed in pieces), bc_count pulls sigma for the
 *      new segment, bc_close (one workgroup) records the step and opens the next.  A sweep of depth d takes d + 1 steps;
 *      its last step finds nothing.  Backward, the host knows the depth and enqueues one ungated launch per level
 *      depth - 1 ... 1 (level 0 is the source alone); bc_delta pulls delta and adds it into bc.
 *      Worst cases: a path pays three launches forward and one backward per level and source, however narrow the level;
 *      a hub's list is pulled by one wave alone, 64 entries at a time; sigma overflows on grids (C(n, n / 2) leaves
 *      float64 near n = 1030).
 *
 *      Measured on an MI355X (DESIGN.md "6p Betweenness centrality"; tools/bc_bench.py, one process per matrix, 4 drawn
 *        sources, sh_bc, as many sh_bfs_levels calls from the same sources -- the forward sweep's floor -- and the host
 *        gold alternating, 5 rounds, device time against the wall time of hostlib.bc_scores), median (min-max) in ms for
 *        the four sources: synth:scircuit (170 998 rows, 958 733 edges): 7.00 (6.98-7.07), 90 steps, 0.044 of the
 *        host's 159.4, 2.98 times the four sh_bfs_levels calls (2.35); R-MAT-18 (262 144 rows, 3 939 181 edges, longest
 *        list 15 918): 14.06 (13.98-14.15), 27 steps, 0.028 of the host's 509.9, 19.3 times the four sh_bfs_levels calls
 *        (0.73: bottom-up levels with an early exit, which a path count cannot use); the 512 x 512 grid (262 144 rows,
 *        1 046 528 edges, depths 662 to 1011, sigma up to 5.5e302): 75.71 (75.68-76.04), 3277 steps, 1.11 times the
 *        host's 68.2 -- the device loses --, 1.12 times the four sh_bfs_levels calls (67.73).  The handle is built in
 *        0.05 s.  More than four sources, graphs below 10^5 rows and graphs whose sigma overflows are unmeasured.
 *        bench.py as parent, new, parent, new on one box: 0.38800, 0.38838, 0.38970, 0.38893 ms per step.
 *
 * sh_bc_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  rows == 0 gives a valid handle.
 * Freeing NULL is SH_OK.  The build runs on the device, once; while it runs it needs the arrays as given, two words per
 * entry and 16 bytes per surviving entry plus 8 per edge for the keys, all released before the call returns.
 * sh_bc_graph_footprint: device bytes held =
 *     12 * (rows + 1) + 24 * rows + 8 * edges + 16 * (edges / 1024 + 1) + 17408.
 * (in_ptr, out_ptr and the level starts; level, order, sigma, delta; in_col and out_col; two piece lists; the control
 * block with a count per workgroup.)  sh_bc_graph_edges: the simple directed edges.  sh_bc_graph_max_list: the longest
 * in- or out-list.
 *
 * sh_bc: sources: a host array of n_sources int32 vertex indices; n_sources == 0 is legal and launches no kernel (with
 * accumulate == 0 bc is still set to +0.0, the sum over no sources).  bc: an sh_vec of >= 2 * rows four-byte elements,
 * 8-byte aligned, read as `rows` little-endian float64 (sh_tri's convention); 2 * rows elements are written, no more.
 * accumulate == 0: bc starts from +0.0; accumulate == 1: the scores are added to what bc holds, so a caller may cut its
 * sources into several calls and get the bits of one call.  sigma (optional, the format of bc) and level (optional,
 * int32, >= rows elements) give the last source's values; without sources they are left alone.  *steps (may be NULL) =
 * the forward steps of all sources.  The per-source arrays are host arrays of n_sources entries, each may be NULL:
 * depth_per_source (int32, the last level that holds a vertex), reached_per_source (int64, the source included),
 * sigma_max_per_source (double), edges_per_source (int64: the out-list entries walked forward, an exact count),
 * ns_per_source and *total_ns device time (hipEvent) as elsewhere.  One handle serves any number of calls, one at a time.
 * rows == 0 gives SH_OK.
 * SH_EINVAL: accumulate outside {0, 1}, n_sources < 0 (the scalars are checked first); NULL arguments (engine, graph, bc,
 * sources when n_sources > 0, out, the arrays); a source outside [0, rows); bc or sigma not aligned to 8 bytes; bc, sigma
 * and level overlapping one another; rows < 0, nnz < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr
 * that decreases; bc or sigma shorter than 2 * rows, level shorter than rows.  All are reported before any device work,
 * with the buffers untouched.
 * NOT covered: several sources per matrix read, weighted shortest paths, edge betweenness, normalisation, the multi-GPU
 * driver, the C++ harness apps.
 */
typedef struct sh_bc_graph sh_bc_graph;
int sh_bc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                       const void *val, sh_bc_graph **out);
int sh_bc_graph_free(sh_engine *e, sh_bc_graph *g);
int sh_bc_graph_footprint(const sh_bc_graph *g, uint64_t *device_bytes);
int sh_bc_graph_edges(const sh_bc_graph *g, int64_t *edges);
int sh_bc_graph_max_list(const sh_bc_graph *g, int64_t *entries);
int sh_bc(sh_engine *e, sh_bc_graph *g, const int32_t *sources, int32_t n_sources, sh_vec *bc, int32_t accumulate,
          sh_vec *sigma, sh_vec *level, int64_t *steps, int32_t *depth_per_source, int64_t *reached_per_source,
          double *sigma_max_per_source, int64_t *edges_per_source, uint64_t *ns_per_source, uint64_t *total_ns);

/* ---- sparse triangular solve: x = T^-1 b by level sets, float64, every sum in one fixed order ----------------------
 * (the reference has no counterpart.  It is the kernel Gauss-Seidel, SSOR and every ILU or IC preconditioner apply: the
 * engine orders (sh_rcm), colours (sh_color), pairs (sh_match) and multiplies (sh_spmv); this solves.  Level scheduling:
 * Anderson, Saad, Int. J. High Speed Computing 1989; on GPUs: Naumov, NVIDIA NVR-2011-001.  The spin-waiting
 * "synchronisation-free" algorithms are out: no kernel here ever waits for another kernel's write.)
 *
 * THE DEFINITION IS PART OF THE ABI.  The matrix is square (rows x rows), given as host CSR with float32 values; uplo
 * selects the triangle (0 lower, 1 upper) and unit == 1 takes the diagonal as one.
 *      Every stored entry (r, c) with 0 <= c < rows takes part, whatever its value: explicit zeros, NaN and infinities
 *      are included and nothing is refused.  Entries of the other triangle and columns out of range are ignored; diagonal
 *      entries are ignored when unit == 1.  Rows need not be sorted.
 *      LIST(r) = the strictly-triangular entries of row r in ascending (column, position as given); parallel entries stay
 *                separate terms (a stable radix sort of the keys (r << bits | c) with the value riding along gives this).
 *      d[r]    = the diagonal entries of r widened to float64 and added left to right, starting from +0.0; a missing
 *                diagonal is +0.0.
 *      level[r] = 0 for an empty list, else 1 + the largest level[c] over the list.  order = the rows in ascending
 *                (level, index); lstart[L] = where level L starts in order.
 *      x[r]    = (b[r] - S_r) / d[r], or b[r] - S_r when unit == 1, with S_r = SUM over LIST(r) of the terms
 *                t_j = (double)val_j * x[col_j].  Each product, the subtraction and the division are rounded once: no fused
 *                multiply-add.  A zero or missing diagonal gives what IEEE gives (inf or NaN); sh_trsv_graph_zero_diag
 *                and _first_zero say how many rows have d[r] == 0 and which is the first, so the caller sees it.
 *      SUM is sh_bc's shape: the list is cut into pieces of 2048 entries, the last one shorter; inside a piece 64 strided
 *      partials, partial[l] = (((+0.0 + t[l]) + t[l + 64]) + t[l + 128]) + ..., folded by the fixed butterfly: for
 *      o = 32, 16, 8, 4, 2, 1: partial[l] = partial[l] + partial[l ^ o] for all l at once; the piece's sum is partial[0];
 *      the piece sums are added left to right, starting from +0.0.  The empty list sums to +0.0.  THE TERMS ARE SIGNED: a
 *      partial starts from +0.0, so it is never -0.0 and padding with +0.0 is exact; a list of up to 8 entries sums to
 *      ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)) with p_k = +0.0 + t_k (not t_k: eight terms of -0.0 sum to +0.0 in
 *      every tier).  A lane (up to 8 entries), a wave (up to a piece) and a wave over several pieces compute ONE function.
 *      With that every comparison is ==, a NaN standing where a NaN stands: tests/trsv_ref.py restates the definition in
 *      numpy and host/src/trsv_solve.cpp in C++.
 *      float32 callers (sh_spmv works in float32): with f32 == 1, b is read as rows float32 and widened, x is written as
 *      float32, rounded once on the way out; later rows read the unrounded float64 value (the handle keeps it).  With
 *      f32 == 0, b and x are rows float64 in 2 * rows four-byte elements, 8-byte aligned (sh_bc's convention).  b and x
 *      may be the same vector.
 *
 *      Schedule (csrc/trsv.hip.h).  sh_trsv_graph_create builds on the device, once: flag and key the entries, one stable
 *      sort, gather values and diagonals; the flipped lists ("who waits for me") serve the analysis only: gated rounds
 *      enqueued ahead of the host in batches (8, 16, 32, 32, ...), a waiting count per row, round L settles its work list
 *      at level L and gives every dependant one atomic decrement per entry, the one lane that sees zero owns the row for
 *      the next round: no compare-and-swap.  One sort of (level << bits | row) gives order.  The flipped lists, the keys
 *      and the work lists are released before the call returns; the host keeps lstart (levels + 1 words).
 *      sh_trsv: one lane per row (64 rows per wave), one owner per x[r], no float atomics.  A wide level is one ungated
 *      launch (trsv_level: the grid sized by the level's width, at most 1024 workgroups, a grid-stride loop).  A run of
 *      consecutive THIN levels is one launch of ONE workgroup (trsv_run) with a workgroup barrier between levels: x is
 *      written and read inside that launch by one workgroup's waves only, by plain stores and loads ordered by the barrier
 *      at workgroup scope; no agent fence, no flag, no spin.  A run holds at most SH_TRSV_RUN = 1024 levels (a level in a
 *      run costs a barrier and a chain of dependent loads, a few microseconds, so a launch stays in the low
 *      milliseconds).  The plan is a host function of lstart, thin and SH_TRSV_RUN alone: a level is thin when it holds at
 *      most `thin` rows; consecutive thin levels form runs, cut at SH_TRSV_RUN; every other level is a launch of its own.
 *      thin == 0 gives one launch per level; thin < 0 means the default, 256; thin > 65536 is refused.  x does not depend
 *      on thin.
 *      Worst cases: a path (a bidiagonal matrix) has `rows` levels of one row: the analysis pays two launches per level,
 *      the solve one barrier per level and one launch per 1024 levels, and a host loop wins; a hub row's list is summed
 *      by one wave alone, 64 entries at a time; the analysis of a matrix with `rows` levels takes `rows` rounds.
 *
 *      Measured on an MI355X (DESIGN.md "6q Sparse triangular solve"; tools/trsv_bench.py, one process per matrix, the
 *        lower triangle with a dominant diagonal, float64, sh_trsv and the host gold alternating, 5 rounds, device time
 *        against the wall time of hostlib.trsv_solve), median in ms: the 2048 x 2048 grid Laplacian as generated
 *        (4 194 304 rows, 4095 levels): thin 0: 18.22, 64: 18.03, 256: 17.53, 1024: 22.39, 4096: 46.25; the host 168.5: the
 *        default is 0.104 of it (a level in a run costs about 3.1 us, a launch of its own 4.45 us).  The same grid
 *        permuted by sh_color's classes (5 levels): 0.076 for every thin, 0.0004 of the host's 174.8.  R-MAT-18 symmetrised
 *        (943 levels, longest list 15 839): 30.68 at thin 256, 0.93 of the host's 32.8: a tie.  synth:scircuit (24
 *        levels): 0.547, 0.069 of the host's 7.90.  The default thin = 256 is the arm that wins on the grid as generated
 *        and loses nothing on the permuted one.  A sweep of SH_TRSV_RUN and a true path are unmeasured.
 *        bench.py as parent, new, parent, new on one box: 0.38762, 0.39065, 0.39172, 0.39044 ms per step.
 *
 * sh_trsv_graph_create: the handle is made from the host CSR arrays alone (no sh_csr).  rows == 0 gives a valid handle
 * and a solve that launches nothing.  Freeing NULL is SH_OK.  While the build runs it needs the arrays as given, two words
 * per entry, about 24 bytes per list entry and 36 per row, all released before the call returns.
 * sh_trsv_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 24 * rows + 8 * entries + 4 * (levels + 1) + 17408.
 * (ptr; d, the float64 x of a float32 call, order and level; col and val; lstart; the analysis' control block with a
 * count per workgroup.)  sh_trsv_graph_entries: the list entries, the diagonal not counted.  _levels, _max_list (the
 * longest list), _max_width (the widest level), _zero_diag (rows with d == 0; always 0 when unit), _first_zero (the
 * smallest such row, -1 if none).  sh_trsv_graph_level: level[r] into an int32 sh_vec of >= rows elements.
 *
 * sh_trsv: *launches = the launches of the call, *runs = how many of them were runs, *levels_in_runs = the levels those
 * held (each may be NULL; they are the plan's, known before anything is launched), *total_ns device time (hipEvent) as
 * elsewhere.  rows elements (f32) or 2 * rows elements of x are written, no more.  One handle serves any number of
 * calls, one at a time.
 * SH_EINVAL: uplo or unit outside {0, 1} (sh_trsv_graph_create), f32 outside {0, 1}, thin > 65536 (the scalars are
 * checked first); NULL arguments; a float64 b or x not aligned to 8 bytes; b and x overlapping without being the same
 * vector; rows < 0, nnz < 0.  SH_ESHAPE: row_ptr[0] != 0, row_ptr[rows] != nnz or a row_ptr that decreases; b or x
 * shorter than rows (f32) or 2 * rows elements; level shorter than rows.  All are reported before any launch, with the
 * buffers untouched.
 * NOT covered: several right-hand sides, the transposed solve, factorisation (ILU, IC), the multi-GPU driver, the C++
 * harness apps.
 */
typedef struct sh_trsv_graph sh_trsv_graph;
int sh_trsv_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const void *val, int32_t uplo, int32_t unit, sh_trsv_graph **out);
int sh_trsv_graph_free(sh_engine *e, sh_trsv_graph *g);
int sh_trsv_graph_footprint(const sh_trsv_graph *g, uint64_t *device_bytes);
int sh_trsv_graph_entries(const sh_trsv_graph *g, int64_t *entries);
int sh_trsv_graph_levels(const sh_trsv_graph *g, int64_t *levels);
int sh_trsv_graph_max_list(const sh_trsv_graph *g, int64_t *entries);
int sh_trsv_graph_max_width(const sh_trsv_graph *g, int64_t *rows);
int sh_trsv_graph_zero_diag(const sh_trsv_graph *g, int64_t *rows);
int sh_trsv_graph_first_zero(const sh_trsv_graph *g, int64_t *row);
int sh_trsv_graph_level(sh_engine *e, sh_trsv_graph *g, sh_vec *level);
int sh_trsv(sh_engine *e, sh_trsv_graph *g, const sh_vec *b, sh_vec *x, int32_t f32, int32_t thin, int64_t *launches,
            int64_t *runs, int64_t *levels_in_runs, uint64_t *total_ns);

/* ---- incomplete LU factorisation without fill, ILU(0): A ~ L U on the pattern of A, by level sets, float64, one fixed order
 * (the reference has no counterpart.  It makes the factor that sh_trsv applies: the engine orders (sh_rcm), colours
 * (sh_color), multiplies (sh_spmv) and solves (sh_trsv); this factorises.  ILU(0): Meijerink, van der Vorst, Math. Comp.
 * 1977; Saad, Iterative Methods for Sparse Linear Systems, algorithm 10.4 (the row-wise IKJ form); by level sets on
 * GPUs: Naumov, NVIDIA NVR-2012-003.  No kernel here ever waits for another kernel's write.)
 *
 * THE DEFINITION IS PART OF THE ABI.  The pattern is square (rows x rows), given as host CSR (row_ptr, col_idx); the
 * float32 values come per call, as an sh_vec of nnz elements in the order of the entries.
 *      SLOTS.  The slots of row r are the distinct columns c with 0 <= c < rows among its entries, in ascending c.  Rows
 *      need not be sorted; entries with a column outside the matrix take no part; nothing is refused, whatever the
 *      values.  a[r, c] = the entries (r, c) in the order given, widened to float64 and added left to right from +0.0
 *      (sh_trsv's rule for d[r]).
 *      RECURRENCE.  Row-wise IKJ, all in float64:
 *          w = a[r, :] on the slots of r
 *          for every slot (r, k) with k < r, ascending k:
 *              w[k] = w[k] / u[k, k]      (the final value of slot (k, k); +0.0 if row k has no diagonal slot)
 *              for every slot (k, j) with j > k, ascending j:
 *                  if (r, j) is a slot: w[j] = w[j] - w[k] * u[k, j]
 *          row r of the factor = w
 *      Every product is rounded once and the subtraction is a second rounding: no fused multiply-add.  l[r, k] = w[k] for
 *      k < r (the unit diagonal of L is not stored), u[r, j] = w[j] for j >= r.  Every slot (r, j) receives its
 *      subtractions in ascending k, one after the other, so the factor is a function of the pattern and the values alone,
 *      whatever the tier, the grid or thin.  A zero, missing or non-finite pivot gives what IEEE gives.  With that every
 *      comparison is ==, a NaN standing where a NaN stands: tests/ilu0_ref.py restates the definition in numpy and
 *      host/src/ilu0_factor.cpp in C++.
 *      OUTPUT.  lu is in the positions of the input entries: lu[p] = the slot's value if entry p is the first entry as
 *      given of its (r, c) group; +0.0 if it is a later entry of the group or its column is outside the matrix.  So
 *      (row_ptr, col_idx, lu) is a CSR matrix that sh_trsv_graph_create(..., uplo = 0, unit = 1) and (..., uplo = 1,
 *      unit = 0) read as exactly L and U.  f32 == 1: nnz float32 elements, each rounded once on the way out (what
 *      sh_trsv_graph_create takes); f32 == 0: 2 * nnz four-byte elements, which is nnz float64, 8-byte aligned.  val and
 *      lu may be the same vector when f32 == 1.  val is not written otherwise.
 *      level[r] = 0 for a row without a lower slot, else 1 + the largest level among its lower slots: sh_trsv_graph_level
 *      of the uplo = 0 handle on the same arrays.
 *      Per call: *zero_pivots = the rows whose pivot u[r, r] compares == 0.0 (a missing diagonal slot counts as +0.0; a
 *      NaN pivot does not count), *first_zero = the smallest such row, -1 if there is none.
 *
 *      Schedule (csrc/ilu0.hip.h).  sh_ilu0_graph_create builds on the device, once, from the pattern alone: sh_trsv's
 *      analysis of the lower triangle gives level, order and lstart (gated rounds of atomic decrements, no
 *      compare-and-swap); the entries inside the matrix are keyed (r << bits | c) with their position riding along, one
 *      stable sort, the heads of the runs of equal keys are the slots.  Per row: its slots (ptr / col), the diagonal slot
 *      or -1, the first upper slot, and its share of work; per slot: its entries in the order given; per input position:
 *      its slot and whether it is the head; one float64 working array w of `entries` elements.
 *      sh_ilu0: one launch loads w from val (ilu0_load), the levels follow sh_trsv's plan -- one ungated launch per wide
 *      level (ilu0_level: the grid sized by the level's width, at most 1024 workgroups, a grid-stride loop), one launch of
 *      ONE workgroup per run of at most 1024 consecutive THIN levels (ilu0_run) with a workgroup barrier between levels
 *      -- and one launch writes lu from w and counts the zero pivots (ilu0_store).  thin has sh_trsv's meaning and range:
 *      thin == 0 gives one launch per level; thin < 0 means the default, 256; thin > 65536 is refused.  A wave takes 64
 *      rows of a level.  A row whose share of work is at most ILU0_LANE_WORK = 256 is eliminated by its lane alone; the
 *      others are taken one at a time by the whole wave, the lanes striding over the upper slots of row k and bisecting
 *      row r's sorted columns; distinct j of one row k are distinct slots, so no two lanes write one word.  Both tiers run
 *      ONE sequence of operations per slot.  One owner per value, no float atomics; w is written and re-read inside a
 *      launch by plain stores and loads, ordered by the barrier at workgroup scope between levels and by a fence at
 *      wavefront scope between the steps of the wave tier; no agent fence, no flag, no spin.  ILU0_LANE_WORK = 256 is the
 *      sweep's choice among 16, 64, 256, 1024 and 4096.
 *      Worst cases: a dense hub row against long rows k is one wave's work alone (no workgroup tier); a path (a
 *      tridiagonal matrix) has `rows` levels of one row, and a host loop wins.
 *      Measured on an MI355X: see DESIGN.md "6r Incomplete LU factorisation" for what was measured and what was not.
 *
 * sh_ilu0_graph_create: the handle is made from the host pattern alone (no sh_csr, no values), and one handle serves any
 * number of sh_ilu0 calls with new values, one at a time: the re-factorisation of a time-stepping or Newton loop.
 * rows == 0 or nnz == 0 give a valid handle and a call that launches nothing (*zero_pivots = rows then: every pivot is
 * missing).  Freeing NULL is SH_OK.
 * sh_ilu0_graph_footprint: device bytes held =
 *     4 * (rows + 1) + 20 * rows + 12 * nnz + 16 * entries + 4 * (levels + 1) + 20.
 * (ptr; dslot, up, the rows' work, order and level; slot_of, head and perm per entry as given; col, gstart and the
 * float64 w per slot, gstart one more; lstart; the figures.)  sh_ilu0_graph_entries: the slots.  _levels, _max_list
 * (the longest row, in slots), _max_width (the widest level), _missing_diag (rows without a diagonal slot),
 * _first_missing (the smallest such row, -1 if none), _work (the look-ups of one factorisation: the sum over every
 * lower slot (r, k) of the upper slots of row k).  sh_ilu0_graph_level: level[r] into an int32 sh_vec of >= rows elements.
 *
 * sh_ilu0: *launches = the launches of the call (ilu0_load where there is a slot, the plan's, ilu0_store), *runs = how
 * many of them were runs, *levels_in_runs = the levels those held (each may be NULL; they are the plan's, known before
 * anything is launched), *zero_pivots and *first_zero as above (each may be NULL), *total_ns device time (hipEvent) as
 * elsewhere.  nnz elements (f32) or 2 * nnz elements of lu are written, no more.
 * SH_EINVAL: f32 outside {0, 1}, thin > 65536 (the scalars are checked first); NULL arguments; a float64 lu not aligned
 * to 8 bytes; val and lu overlapping without being the same float32 vector; rows < 0, nnz < 0.  SH_ESHAPE: row_ptr[0] != 0,
 * row_ptr[rows] != nnz or a row_ptr that decreases; val shorter than nnz elements, lu shorter than nnz (f32) or 2 * nnz;
 * level shorter than rows.  All are reported before any launch, with the buffers untouched.
 * NOT covered: IC(0), ILU(k), ILUT, pivoting and diagonal shifts; refreshing a sh_trsv handle's values on the device (the
 * factor goes through the host once per factorisation); a workgroup tier for hub rows; the multi-GPU driver.
 */
typedef struct sh_ilu0_graph sh_ilu0_graph;
int sh_ilu0_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         sh_ilu0_graph **out);
int sh_ilu0_graph_free(sh_engine *e, sh_ilu0_graph *g);
int sh_ilu0_graph_footprint(const sh_ilu0_graph *g, uint64_t *device_bytes);
int sh_ilu0_graph_entries(const sh_ilu0_graph *g, int64_t *entries);
int sh_ilu0_graph_levels(const sh_ilu0_graph *g, int64_t *levels);
int sh_ilu0_graph_max_list(const sh_ilu0_graph *g, int64_t *entries);
int sh_ilu0_graph_max_width(const sh_ilu0_graph *g, int64_t *rows);
int sh_ilu0_graph_missing_diag(const sh_ilu0_graph *g, int64_t *rows);
int sh_ilu0_graph_first_missing(const sh_ilu0_graph *g, int64_t *row);
int sh_ilu0_graph_work(const sh_ilu0_graph *g, int64_t *lookups);
int sh_ilu0_graph_level(sh_engine *e, sh_ilu0_graph *g, sh_vec *level);
int sh_ilu0(sh_engine *e, sh_ilu0_graph *g, sh_vec *val, sh_vec *lu, int32_t f32, int32_t thin, int64_t *launches,
            int64_t *runs, int64_t *levels_in_runs, int64_t *zero_pivots, int64_t *first_zero, uint64_t *total_ns);

#ifdef __cplusplus
}
#endif
#endif /* SPARSEHARNESS_HIP_H_ */
