// engine.hip -- implementation of the C ABI declared in
// include/sparseharness_hip.h: a thin hipMalloc / hipMemcpyAsync / hipStream
// layer (replacing the reference's OpenCL context + CLMemoryManager,
// inc/harness.h:13-82, inc/cl_memory_manager.h:6-29) plus the launch logic of
// the native CSR SpMV kernels (kernels.hip.h).
//
// No CPU fallback: every compute entry point needs a live HIP device.
#include "../../include/sparseharness_hip.h"
#include "kernels.hip.h"
#include "bits.hip.h"
#include "multi.hip.h"
#include "msbfs.hip.h"
#include "frontier.hip.h"
#include "bfs.hip.h"
#include "sssp.hip.h"
#include "scc.hip.h"
#include "wcc.hip.h"
#include "tri.hip.h"
#include "core.hip.h"
#include "truss.hip.h"
#include "color.hip.h"
#include "msf.hip.h"
#include "match.hip.h"
#include "rcm.hip.h"
#include "bc.hip.h"
#include "trsv.hip.h"
#include "ilu0.hip.h"
#include "plan_common.h"
#include "plan_host.h"
#include "dev_arrays.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <chrono>

using namespace sh;

// The words a batch of launches writes on the device and their pinned copy.  Each half is allocated when first missing.
template <class T>
struct BatchWords {
  T *d = nullptr, *h = nullptr;
  size_t size = 0;   // the bytes behind each half
  hipError_t open(size_t bytes) {
    size = bytes;
    hipError_t r = d ? hipSuccess : hipMalloc((void **)&d, bytes);
    if (r == hipSuccess && !h) r = hipHostMalloc((void **)&h, bytes, hipHostMallocDefault);
    return r;
  }
  void close() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
  }
};
struct DenseLoopState {   // what run_dense_batches and its four users keep between calls
  hipEvent_t ev[9] = {};          // one per launch of a batch, and one in front
  BatchWords<int32_t> flags;      // sh_iterate: 64 B, the convergence flags of a batch (the pinned half is the engine's from the start)
  BatchWords<int32_t> mflags;     // sh_iterate_multi: MULTI_FLAG_WORDS per-column flags of a batch
  BatchWords<uint32_t> bstate;    // sh_bits_iterate: BITS_STATE_WORDS changed words and level counts of a batch
  void close() {
    flags.close(); mflags.close(); bstate.close();
    for (auto e : ev) if (e) (void)hipEventDestroy(e);
  }
};

struct sh_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DenseLoopState dense;
  char name[256] = {0};
  int n_cus = 256;
  std::string err;
};

// A matrix handle is up to three device layouts and the state of its piece reports.  Each part owns its arrays
// (dev_arrays.h): dropping a layout is assigning an empty one, and freeing the handle is deleting it.
struct StreamLayout {   // the CSR-stream plan (plan A); its first three arrays are also the device builders' input
  DevArrays dev;
  int32_t *d_row_ptr = nullptr, *d_col = nullptr;
  uint32_t *d_val = nullptr;
  int32_t *d_blk_row = nullptr;
  LongSeg *d_segs = nullptr;
  LongRow *d_long = nullptr;
  uint32_t *d_partial = nullptr;
  uint32_t *d_partial_multi = nullptr;   // sh_spmm: SPMM_MAX_WIDTH partials per long-row segment
  int32_t n_stream = 0, n_segs = 0, n_long = 0;
};
struct TiledLayout {   // the x-tiled two-phase plan (kernels.hip.h); built when plan == PLAN_TILED
  DevArrays dev;
  RowBin *d_bins = nullptr;
  int32_t n_bins = 0;
  TileChunk *d_chunks = nullptr;
  int32_t n_chunks = 0;
  uint32_t *d_tval = nullptr, *d_gdest = nullptr, *d_gblk = nullptr, *d_P = nullptr, *d_obase = nullptr;
  int32_t *d_ptab = nullptr;
  uint16_t *d_ptile = nullptr;     // per piece: its column tile
  int tcols = TCOLS;               // columns per x tile: TCOLS, or TCOLS_WIDE for a wide layout (plan_common.h::pick_tile_cols)
  uint64_t *d_fmask = nullptr;     // wide layouts: the fold flags, one mask word per block of d_obase
  int32_t *d_ptab_live = nullptr;  // per launch of a semiring with absorbing words: ptab with the pieces of dead tiles marked (tiled_mark_dead)
  uint32_t *d_tile_live = nullptr; // per column tile: phase 1 found a word of x that is not absorbing
  int64_t n_pieces = 0;
  uint8_t *d_tcode = nullptr;    // value coding: one-byte dictionary codes instead of d_tval
  uint32_t *d_vdict = nullptr;   // [VDICT] original bit patterns
  int n_vdict = 0;               // 0 = values stored raw
  int code_bits = 0;             // 8 or 4 when n_vdict != 0
  int n_vdict_used = 0;          // distinct values found (<= VDICT)
  uint16_t *d_tcol = nullptr, *d_pslot = nullptr;
  LongRow *d_tlong = nullptr;   // heavy rows (pre-reduced in phase 1)
  int32_t n_tlong = 0;
  uint32_t *d_tpartial = nullptr;
  int32_t *d_lrp = nullptr;     // light row offsets, bit 31 = heavy row
  int64_t light_len = 0, light_entries = 0;   // light part of the stream (padding included) / light entries of the matrix
  int64_t stream_len = 0, p_len = 0;          // stream entries in all / products in P
  int fold = 0;                               // phase 1 folds a row's entries inside a tile into one product
  bool skip_minplus = false;                  // every |value| < 2^103: FLT_MAX + |a| == FLT_MAX, so tiles of unreached x words may be skipped
  std::vector<int32_t> bin_r0;                // first row of every row bin (host copy: piece reporting)
};
struct BitsLayout {   // the (or,and) semiring on bits (bits.hip.h); built when sh_plan_options::or_and_bits asks for it
  DevArrays dev;
  BitsItem *d_bits_items = nullptr;
  uint32_t *d_bits_ent = nullptr, *d_bits_partial = nullptr;
  int32_t *d_bits_sub = nullptr, *d_bits_rr0 = nullptr;
  uint64_t *d_xbits = nullptr;
  int32_t n_bits_items = 0, bits_ct = 0;
  int64_t bits_entries = 0;
};
struct PieceReport {   // piece reporting (sh_spmv_step_pieces); made whole by the first such launch (open_piece_report)
  DevArrays dev;                              // (not part of the footprint)
  uint32_t *d_done = nullptr, *h_done = nullptr;   // arrival counters / host-visible round words (pinned)
  PieceDev *d_pcs = nullptr;                  // the pieces' geometry as the kernels read it (device copy of pcs_host)
  PieceDev pcs_host{};                        // what d_pcs holds (rewritten only when a call brings another geometry)
  bool pcs_valid = false;
  uint32_t round = 0;                         // reporting launches so far
  uint32_t last_expected = 0;                 // arrivals per piece the latest reporting launch waits for (sh_csr_piece_state)
  ~PieceReport() {
    if (h_done) (void)hipHostFree(h_done);
  }
};

struct sh_csr {
  int64_t rows = 0, cols = 0, nnz = 0;
  int plan = 0;
  bool tuned = false;           // plan confirmed by timing both at upload (autotune_plan)
  float tuned_ms[2] = {0, 0};   // [stream, tiled]
  StreamLayout stream;
  TiledLayout tiled;
  BitsLayout bits;
  std::unique_ptr<PieceReport> pieces;
  bool bits_only = false;                     // no other plan was built: only SH_OR_AND_I32 launches are served
  bool built_on_device = false;               // the tiled layout was built by plan_gpu.hip
  int placement_tries = 1;                    // placements of the big arrays timed at upload (tune_placement)
  float placement_ms[2] = {0, 0};             // [first placement, the one kept]
  std::string build_note;                     // why the device builder was not used / fell back (empty: nothing to say)
  size_t device_bytes() const { return stream.dev.bytes + tiled.dev.bytes + bits.dev.bytes; }
};
enum { PLAN_STREAM = 0, PLAN_TILED = 1 };
constexpr int SPMM_MAX_WIDTH = 32;   // widest sh_spmm

struct sh_vec {
  void *d = nullptr;
  int64_t n = 0;
  bool owned = false;
};

static thread_local std::string g_create_err;

static int fail(sh_engine *e, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e)
    e->err = buf;
  else
    g_create_err = buf;
  return code;
}

#define HIP_TRY(e, call)                                                        \
  do {                                                                          \
    hipError_t _r = (call);                                                     \
    if (_r != hipSuccess)                                                       \
      return fail((e), _r == hipErrorOutOfMemory ? SH_ENOMEM : SH_EHIP,         \
                  "%s failed: %s (%s:%d)", #call, hipGetErrorString(_r),        \
                  __FILE__, __LINE__);                                          \
  } while (0)

// What every sh_*_free is: the stream drains (copies from host arrays may be in flight), then the handle goes with all it owns.
template <class H>
static int free_handle(sh_engine *e, H *h) {
  if (!h)
    return SH_OK;
  if (e) {
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
  }
  delete h;
  return SH_OK;
}

#define RC_TRY(call) do { if (const int _rc = (call)) return _rc; } while (0)   // for the functions that set the message themselves

// Device array of `bytes` (+ slack for the kernels' wide loads) owned by `own` and counted in its footprint, filled from
// `host` when given.  Enqueued only: `host` lives until the stream has been synchronised.
template <class T>
static int dev_array(sh_engine *e, DevArrays &own, T **p, const void *host, size_t bytes, size_t slack) {
  HIP_TRY(e, own.alloc_exact(p, bytes + slack));
  if (host && bytes > 0)
    HIP_TRY(e, hipMemcpyAsync(*p, host, bytes, hipMemcpyHostToDevice, e->stream));
  return SH_OK;
}

// One big array of the tiled layout: handed over by the device builder (`dev`, n_dev elements and the slack behind
// them) or uploaded from the host builder's vector.
template <class T, class D>
static int plan_array(sh_engine *e, sh_csr *m, T **p, D *&dev, size_t n_dev, const std::vector<T> &host, size_t slack) {
  if (!m->built_on_device) return dev_array(e, m->tiled.dev, p, host.data(), host.size() * sizeof(T), slack);
  *p = (T *)dev;
  m->tiled.dev.adopt(dev, n_dev * sizeof(T) + slack);
  dev = nullptr;
  return SH_OK;
}

// The describe string of a tiled layout (sh_csr_describe; the tools build also prints it for a layout that was only
// built on the host).  A wide layout says its tile width; a narrow layout's string is what it always was.
static void describe_tiled(char *buf, size_t buflen, int64_t cols, int tcols, int n_vdict, int code_bits, int vdict_used, long long chunks,
                           long long bins, long long heavy_rows, int64_t stream_len, int64_t light_entries, int64_t p_len, bool fold) {
  char vals[32], tile[24] = "";
  if (n_vdict) snprintf(vals, sizeof vals, "dict%d(%d)", code_bits, vdict_used);
  else snprintf(vals, sizeof vals, "raw");
  if (tcols != TCOLS) snprintf(tile, sizeof tile, " tile=%d", tcols);
  snprintf(buf, buflen, "tiled values=%s tiles=%lld%s chunks=%lld bins=%lld heavy_rows=%lld stream=%.1fM light=%.1fM products=%.1fM%s", vals,
           (long long)((cols + tcols - 1) / tcols), tile, chunks, bins, heavy_rows, stream_len / 1e6, light_entries / 1e6, p_len / 1e6,
           fold ? " folded" : "");
}

extern "C" {

int sh_abi_version(void) { return SH_ABI_VERSION; }

int sh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

const char *sh_last_error(const sh_engine *e) {
  return e ? e->err.c_str() : g_create_err.c_str();
}

static int engine_create(int device, void *stream, bool borrow, sh_engine **out) {
  if (!out)
    return fail(nullptr, SH_EINVAL, "sh_engine_create: out is NULL");
  *out = nullptr;
  int n = sh_device_count();
  if (n <= 0)
    return fail(nullptr, SH_ENODEVICE,
                "no HIP device available: the sparseharness HIP engine has no CPU fallback");
  if (device < 0 || device >= n)
    return fail(nullptr, SH_ENODEVICE, "device ordinal %d out of range [0,%d)", device, n);
  sh_engine *e = new (std::nothrow) sh_engine();
  if (!e)
    return fail(nullptr, SH_ENOMEM, "out of host memory");
  e->device = device;
  hipError_t r = hipSetDevice(device);
  if (r == hipSuccess) {
    if (borrow) {
      e->stream = (hipStream_t)stream;
    } else {
      r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
      e->own_stream = true;
    }
  }
  if (r == hipSuccess) r = hipEventCreate(&e->ev0);
  if (r == hipSuccess) r = hipEventCreate(&e->ev1);
  if (r == hipSuccess) r = hipHostMalloc((void **)&e->dense.flags.h, 64, hipHostMallocDefault);
  if (r == hipSuccess) memset(e->dense.flags.h, 0, 64);
  hipDeviceProp_t prop;
  if (r == hipSuccess) r = hipGetDeviceProperties(&prop, device);
  // The runtime loads this file's code object when one of its kernels is first asked for, and that takes milliseconds
  // that grow with every kernel the file gains.  Asking here keeps them out of the first launch a caller times (the apps
  // time every trial, and a first trial above their timeout ends the run: host/app/spmv.cpp).
  hipFuncAttributes attr;
  if (r == hipSuccess) r = hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(wl_edge_ends));
  if (r != hipSuccess) {
    int rc = fail(nullptr, SH_EHIP, "engine init failed: %s", hipGetErrorString(r));
    delete e;
    return rc;
  }
  snprintf(e->name, sizeof e->name, "%s (%s)", prop.name[0] ? prop.name : "AMD GPU", prop.gcnArchName);
  e->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  *out = e;
  return SH_OK;
}

int sh_engine_create(int device_ordinal, sh_engine **out) {
  return engine_create(device_ordinal, nullptr, false, out);
}
int sh_engine_create_on_stream(int device_ordinal, void *hip_stream, sh_engine **out) {
  return engine_create(device_ordinal, hip_stream, true, out);
}

int sh_engine_destroy(sh_engine *e) {
  if (!e)
    return SH_OK;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  e->dense.close();
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
  return SH_OK;
}

int sh_engine_device_name(sh_engine *e, char *buf, size_t buflen) {
  if (!e || !buf || buflen == 0)
    return fail(e, SH_EINVAL, "sh_engine_device_name: bad argument");
  snprintf(buf, buflen, "%s", e->name);
  return SH_OK;
}

int sh_engine_max_alloc(sh_engine *e, uint64_t *bytes) {
  if (!e || !bytes)
    return fail(e, SH_EINVAL, "sh_engine_max_alloc: bad argument");
  size_t fr = 0, tot = 0;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemGetInfo(&fr, &tot));
  *bytes = fr;
  return SH_OK;
}

int sh_engine_synchronize(sh_engine *e) {
  if (!e)
    return SH_EINVAL;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return SH_OK;
}


static int dispatch(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x, const sh_vec *y,
                    const void *alpha, const void *beta, sh_vec *out, StepDev st);

// The zeroed x and the out vector that the timings at upload launch on (autotune_plan, tune_placement); released
// with the object.
struct TrialVectors {
  DevArrays dev;
  sh_vec x, out;
  bool open(sh_engine *e, const sh_csr *m) {
    const size_t xbytes = (size_t)std::max<int64_t>(m->cols, 1) * 4;
    if (dev.alloc_exact(&x.d, xbytes) != hipSuccess || dev.alloc_exact(&out.d, (size_t)std::max<int64_t>(m->rows, 1) * 4) != hipSuccess)
      return false;
    x.n = m->cols; out.n = m->rows;
    (void)hipMemsetAsync(x.d, 0, xbytes, e->stream);
    return true;
  }
  // ms per (+,x) launch on the matrix's current plan and placement: `warm` launches, then `reps` back to back as one
  // interval; < 0: a call failed
  float time_launches(sh_engine *e, const sh_csr *m, int warm, int reps) {
    const float one = 1.0f, zero = 0.0f;
    float ms = 0;
    bool ok = true;
    for (int rep = -warm; rep < reps && ok; rep++)
      ok = (rep != 0 || hipEventRecord(e->ev0, e->stream) == hipSuccess) &&
           dispatch(e, SH_PLUS_TIMES_F32, m, &x, nullptr, &one, &zero, &out, StepDev{nullptr, nullptr, 0, 0.0}) == SH_OK;
    ok = ok && hipEventRecord(e->ev1, e->stream) == hipSuccess && hipEventSynchronize(e->ev1) == hipSuccess &&
         hipEventElapsedTime(&ms, e->ev0, e->ev1) == hipSuccess;
    return ok ? ms / reps : -1.f;
  }
};

// The size rule picks the tiled plan for every large matrix, but a large matrix whose columns are
// local (banded, FEM-like) keeps its x window in L2 and streams 8 B/entry under plan A, which the
// tiled plan cannot match.  So when the rule says "tiled" and nobody forced a plan, both are
// timed once on the device (x = 0: the memory behaviour of a launch does not depend on the values)
// and plan A is kept only if it is clearly faster -- 10 % -- so that near-ties, where the two
// plans' float rounding of heavy rows could differ, always resolve the same way.
static void autotune_plan(sh_engine *e, sh_csr *m) {
  TrialVectors v;
  if (!v.open(e, m)) return;
  float ms[2] = {0, 0};
  bool ok = true;
  for (int plan : {PLAN_TILED, PLAN_STREAM}) {
    m->plan = plan;
    for (int rep = 0; rep < 3 && ok; rep++) {   // one warm-up, then the faster of two
      const float t = v.time_launches(e, m, 0, 1);
      ok = t >= 0;
      if (ok && rep > 0) ms[plan] = (rep == 1) ? t : std::min(ms[plan], t);
    }
  }
  (void)hipStreamSynchronize(e->stream);
  m->plan = (ok && ms[PLAN_STREAM] < 0.9f * ms[PLAN_TILED]) ? PLAN_STREAM : PLAN_TILED;
  // the layout of the plan that lost is of no further use
  if (m->plan == PLAN_STREAM) m->tiled = TiledLayout();
  else m->stream = StreamLayout();
  m->tuned = ok;
  m->tuned_ms[0] = ms[PLAN_STREAM];
  m->tuned_ms[1] = ms[PLAN_TILED];
}

// Where hipMalloc happens to put the big arrays moves the SpMV time of one and the same layout by +-2 % (stable for the
// life of the allocation: profiles/r03_placement_probe_*.json; no alignment or stride rule was found behind it).  So the
// upload of a large matrix tries `tries` placements of the four big streams -- the product array, the column codes, the
// value codes and the slots -- times (+,x) launch pairs on each (four back to back after a warm-up)
// and keeps the fastest; the others are freed.  All candidates stay allocated until the choice is made, or the allocator
// would hand the same place out again.  Costs about 5 ms and one copy of the arrays per try, at upload only.
static void tune_placement(sh_engine *e, sh_csr *m, int tries) {
  TiledLayout &t = m->tiled;
  if (tries <= 1 || m->plan != PLAN_TILED || t.n_bins <= 0 || t.n_chunks <= 0) return;
  TrialVectors v;
  if (!v.open(e, m)) return;
  struct Slot { void **field; bool copy; };
  const Slot slots[4] = {{(void **)&t.d_P, false},   // (rewritten by every launch)
                         {(void **)&t.d_tcol, true},
                         {t.n_vdict ? (void **)&t.d_tcode : (void **)&t.d_tval, true},
                         {(void **)&t.d_pslot, true}};
  auto time_it = [&]() { return v.time_launches(e, m, 1, 4); };   // (four launch pairs back to back: the steady state of a loop)
  struct Set { void *p[4]; float ms; };
  std::vector<Set> sets;
  Set cur{{*slots[0].field, *slots[1].field, *slots[2].field, *slots[3].field}, time_it()};
  sets.push_back(cur);
  size_t best = 0;
  size_t bytes[4], set_bytes = 0;   // (as allocated at upload: the owner remembers)
  for (int i = 0; i < 4; i++) set_bytes += bytes[i] = t.dev.size_of(cur.p[i]);
  for (int k = 1; k < tries && sets[0].ms > 0; k++) {
    size_t fr = 0, tot = 0;   // (the candidates are all held until the end: never take more than half of what is free)
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < 2 * set_bytes + ((size_t)1 << 30)) break;
    Set fresh{{nullptr, nullptr, nullptr, nullptr}, -1.f};
    bool ok = true;
    for (int i = 0; i < 4 && ok; i++) {
      ok = hipMalloc(&fresh.p[i], bytes[i]) == hipSuccess;
      if (ok && slots[i].copy)
        ok = hipMemcpyAsync(fresh.p[i], sets[0].p[i], bytes[i], hipMemcpyDeviceToDevice, e->stream) == hipSuccess;
    }
    if (!ok) {
      (void)hipStreamSynchronize(e->stream);
      for (void *q : fresh.p) if (q) (void)hipFree(q);
      break;
    }
    for (int i = 0; i < 4; i++) *slots[i].field = fresh.p[i];
    fresh.ms = time_it();
    sets.push_back(fresh);
    if (fresh.ms > 0 && fresh.ms < sets[best].ms) best = sets.size() - 1;
  }
  (void)hipStreamSynchronize(e->stream);
#ifdef SH_PLAN_EMULATE
  if (getenv("SH_PLACEMENT_LOG"))
    for (size_t k = 0; k < sets.size(); k++)
      fprintf(stderr, "[placement] %2zu  P %p  tcol %p  tcode %p  pslot %p  %.4f ms%s\n", k, sets[k].p[0], sets[k].p[1], sets[k].p[2], sets[k].p[3],
              sets[k].ms, k == best ? "  <- kept" : "");
#endif
  for (int i = 0; i < 4; i++) {   // the layout owns the set kept; every other one goes
    t.dev.replace(sets[0].p[i], sets[best].p[i]);
    *slots[i].field = sets[best].p[i];
  }
  for (size_t k = 0; k < sets.size(); k++)
    if (k != best)
      for (void *q : sets[k].p) (void)hipFree(q);
  m->placement_tries = (int)sets.size();
  m->placement_ms[0] = sets[0].ms; m->placement_ms[1] = sets[best].ms;
}

static int choose_plan(const sh_plan_options &opt, int64_t cols, int64_t nnz) {
  if (opt.plan == 1) return PLAN_STREAM;
  if (opt.plan == 2) return PLAN_TILED;
  // auto: x beyond the per-XCD L2 (4 MiB) makes global gathers line-miss bound
  return (cols > (1 << 20) && nnz >= (1 << 22)) ? PLAN_TILED : PLAN_STREAM;
}

// Estimated HBM bytes per row under the plan sh_csr_upload would choose, as a prefix sum: what row-range sharding
// balances on (a shard full of heavy rows would otherwise finish early while the others still stream).  The weights
// follow the tiled plan's traffic: an entry of a light row ~3 B of stream + ~10.5 B for the product that travels
// through P (pair folding saves a seventh of them), an entry of a heavy row ~3 B of stream + the padding of its
// strips; a row costs ~12 B (offsets, result) either way.  CSR-stream plan: 8 B per entry + 12 B per row.
int sh_plan_row_work(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const sh_plan_options *opt_p,
                     uint64_t *work_prefix) {
  if (rows < 0 || cols < 0 || nnz < 0 || !row_ptr || !work_prefix)
    return SH_EINVAL;
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  const bool tiled = choose_plan(opt, cols, nnz) == PLAN_TILED && nnz > 0;
  // (the values are not known here: the tile width a matrix of this size gets unless it needs two-byte codes)
  const int tcols = pick_tile_cols(true, 8, nnz);
  const int CT = (int)std::max<int64_t>(1, (cols + tcols - 1) / tcols);
  const int64_t heavy_thr = std::min<int64_t>(TBIN / 4, std::max<int64_t>(512, (int64_t)std::max(1, opt.heavy_per_tile) * CT));
  uint64_t acc = 0;
  work_prefix[0] = 0;
  for (int64_t r = 0; r < rows; r++) {
    const int64_t d = (int64_t)row_ptr[r + 1] - row_ptr[r];
    if (d < 0) return SH_ESHAPE;
    acc += 12u + (uint64_t)(!tiled ? 8 * d : (d >= heavy_thr ? 4 * d : 12 * d));
    work_prefix[r + 1] = acc;
  }
  return SH_OK;
}

// sh_plan_options::build == 0: the tiled layout is built on the device from this many entries on (a 200 M-entry matrix:
// 0.11 s instead of 0.72 s per upload, profiles/r03_build_probe.json); below, the host builder's microseconds beat the
// device builder's ~40 allocations and launches.
static constexpr int64_t DEVICE_BUILD_MIN_NNZ = 1 << 20;

void sh_plan_options_default(sh_plan_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->autotune = 1;
  o->heavy_per_tile = 8;
  o->chunk = 0;   // auto (see build_tiled_plan)
  o->xcd_order = 1;
  o->fold = 1;
  o->or_and_bits = 0;
}

void sh_plan_options_from_env(sh_plan_options *o) {
  if (!o) return;
  sh_plan_options_default(o);
  auto num = [](const char *name, int32_t &dst) { if (const char *v = getenv(name)) dst = atoi(v); };
  if (const char *v = getenv("SH_PLAN")) o->plan = !strcmp(v, "stream") ? 1 : (!strcmp(v, "tiled") ? 2 : 0);
  if (const char *v = getenv("SH_AUTOTUNE")) o->autotune = v[0] != '0';
  if (const char *v = getenv("SH_VALCODE")) o->value_coding = !strcmp(v, "off") ? -1 : (!strcmp(v, "8") ? 8 : 0);
  num("SH_BUILD_THREADS", o->build_threads);
  num("SH_HEAVY_PER_TILE", o->heavy_per_tile);
  num("SH_CHUNK", o->chunk);
  if (const char *v = getenv("SH_XCD_ORDER")) o->xcd_order = v[0] != '0';
  if (const char *v = getenv("SH_FOLD")) o->fold = v[0] != '0';
  num("SH_OR_AND_BITS", o->or_and_bits);
  num("SH_PLACEMENT_TRIES", o->placement_tries);
  if (const char *v = getenv("SH_BUILD")) o->build = !strcmp(v, "host") ? 1 : ((!strcmp(v, "device") || !strcmp(v, "gpu")) ? 2 : 0);
}

int sh_csr_upload(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr,
                  const int32_t *col_idx, const void *val, sh_csr **out) {
  sh_plan_options opt;
  sh_plan_options_from_env(&opt);   // the SH_* knobs: read once per upload, never at launch time
  return sh_csr_upload_ex(e, rows, cols, nnz, row_ptr, col_idx, val, &opt, out);
}

// The host arrays of an upload, as the caller gave them.
struct HostCsr {
  int64_t rows, cols, nnz;
  const int32_t *row_ptr, *col_idx;
  const uint32_t *val;
};

// row_ptr / col_idx / val as they are: plan A's arrays, and the device builders' input (nothing to do when they are there)
static int upload_csr_arrays(sh_engine *e, sh_csr *m, const HostCsr &h) {
  StreamLayout &s = m->stream;
  if (s.d_row_ptr) return SH_OK;
  const int64_t padded = ((h.nnz + 3) & ~int64_t(3)) + 4;   // the tail is padded so that 16-byte loads at the end stay in bounds
  RC_TRY(dev_array(e, s.dev, &s.d_row_ptr, h.row_ptr, (h.rows + 1) * 4, 0));
  RC_TRY(dev_array(e, s.dev, &s.d_col, nullptr, padded * 4, 0));
  RC_TRY(dev_array(e, s.dev, &s.d_val, nullptr, padded * 4, 0));
  HIP_TRY(e, hipMemsetAsync(s.d_col + (padded - 8 > 0 ? padded - 8 : 0), 0xFF, (padded >= 8 ? 8 : padded) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(s.d_val + (padded - 8 > 0 ? padded - 8 : 0), 0, (padded >= 8 ? 8 : padded) * 4, e->stream));
  if (h.nnz > 0) {
    HIP_TRY(e, hipMemcpyAsync(s.d_col, h.col_idx, h.nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.d_val, h.val, h.nnz * 4, hipMemcpyHostToDevice, e->stream));
  }
  return SH_OK;
}

static void drop_stream_layout(sh_engine *e, sh_csr *m) {
  if (!m->stream.d_row_ptr) return;
  (void)hipStreamSynchronize(e->stream);
  m->stream = StreamLayout();
}

// The bit-blocked layout of the (or,and) semiring: built on the device from the CSR arrays (`device_build`) or, also when
// a device step fails, on the host.  Leaves m->bits empty when the layout does not apply to the matrix.
static int build_bits_layout(sh_engine *e, sh_csr *m, const HostCsr &h, const sh_plan_options &opt, bool device_build) {
  BitsHost bh;
  int built = -1;   // 1 built, 0 the layout does not apply, -1 not tried / a device step failed: the host builder
  uint32_t *dev_ent = nullptr;
  if (device_build) {
    RC_TRY(upload_csr_arrays(e, m, h));
    std::string why;
    built = build_bits_plan_gpu(e->stream, h.rows, h.cols, h.nnz, m->stream.d_row_ptr, m->stream.d_col, m->stream.d_val, bh, &dev_ent, why);
    if (built != 1) { m->build_note = why; bh = BitsHost(); }
  }
  if (built < 0) built = build_bits_plan(h.rows, h.cols, h.nnz, h.row_ptr, h.col_idx, h.val, opt, bh) ? 1 : 0;
  if (built != 1) return SH_OK;
  BitsLayout &b = m->bits;
  b.n_bits_items = (int32_t)bh.items.size();
  b.bits_ct = bh.n_ct;
  b.bits_entries = bh.entries;
  m->bits_only = opt.or_and_bits >= 2;
  if (dev_ent) { b.d_bits_ent = dev_ent; b.dev.adopt(dev_ent, (size_t)bh.ent_len * 4 + SLACK_WIDE); m->built_on_device = true; }
  else RC_TRY(dev_array(e, b.dev, &b.d_bits_ent, bh.ent.data(), bh.ent.size() * 4, SLACK_WIDE));
  RC_TRY(dev_array(e, b.dev, &b.d_bits_items, bh.items.data(), bh.items.size() * sizeof(BitsItem), 32));
  RC_TRY(dev_array(e, b.dev, &b.d_bits_sub, bh.bsub.data(), bh.bsub.size() * 4, 16));
  RC_TRY(dev_array(e, b.dev, &b.d_bits_rr0, bh.rr_item0.data(), bh.rr_item0.size() * 4, 0));
  RC_TRY(dev_array(e, b.dev, &b.d_xbits, nullptr, (size_t)bh.n_ct * (BITS_BC / 8), 0));
  RC_TRY(dev_array(e, b.dev, &b.d_bits_partial, nullptr, (size_t)std::max<size_t>(bh.items.size(), 1) * (BITS_BR / 8), 0));
  HIP_TRY(e, hipStreamSynchronize(e->stream)); // host vectors die at return
  return SH_OK;
}

// Where the tiled layout is built (sh_plan_options::build): on the device from the CSR arrays (plan_gpu.hip; the
// default), or by the host builder -- also the fallback when a device step fails.  Same bytes either way.
// *tiled: the layout is in th (and, built on the device, its big arrays in td).
static int build_tiled_layout(sh_engine *e, sh_csr *m, const HostCsr &h, const sh_plan_options &opt, bool device_build,
                              TiledHost &th, TiledDevArrays &td, bool *tiled) {
  bool want_tiled = choose_plan(opt, h.cols, h.nnz) == PLAN_TILED && h.nnz > 0;
  *tiled = false;
  if (want_tiled && device_build) {
    RC_TRY(upload_csr_arrays(e, m, h));
    lap("H2D of the CSR arrays");
    std::string why;
    const int g = build_tiled_plan_gpu(e->stream, h.rows, h.cols, h.nnz, h.row_ptr, m->stream.d_row_ptr, m->stream.d_col, m->stream.d_val, opt,
                                       e->n_cus, th, td, why);
    lap("device build");
    if (g == 1) {
      *tiled = true;
      m->built_on_device = true;
    } else {
      td.release();
      th = TiledHost();
      m->build_note = why;
      if (g == 0) want_tiled = false;   // the layout does not suit this matrix: the host builder would refuse as well
    }
  }
#ifdef SH_PLAN_EMULATE
  if (want_tiled && !*tiled) {   // (tools builds: sh_debug_held_at_host_build)
    g_debug_held_at_host_build = 0;
    for (const void *p : {(const void *)td.tcol, (const void *)td.pslot, (const void *)td.tcode, (const void *)td.tval, (const void *)td.gdest,
                          (const void *)td.gblk, (const void *)td.obase, (const void *)td.lrp, (const void *)td.ptab, (const void *)td.ptile, (const void *)td.fmask})
      if (p) g_debug_held_at_host_build++;
  }
#endif
  if (want_tiled && !*tiled)
    *tiled = build_tiled_plan(h.rows, h.cols, h.nnz, h.row_ptr, h.col_idx, h.val, opt, e->n_cus, th);
  return SH_OK;
}

// The tiled layout on the device: the small tables from th, the big arrays from td or th (plan_array).
static int upload_tiled_layout(sh_engine *e, sh_csr *m, const sh_plan_options &opt, const TiledHost &th, TiledDevArrays &td) {
  TiledLayout &t = m->tiled;
  t.n_bins = (int32_t)th.bins.size();
  t.n_chunks = (int32_t)th.chunks.size();
  t.n_tlong = (int32_t)th.heavy.size();
  t.light_len = th.light_len;
  t.stream_len = th.stream_len;
  t.p_len = th.p_len;
  t.light_entries = th.light_entries;
  t.tcols = th.tcols;
  t.fold = opt.fold != 0 && (th.tcols != TCOLS || TCOL_FOLD != 0);
  t.bin_r0.reserve(th.bins.size());
  for (const RowBin &b : th.bins) t.bin_r0.push_back(b.r0);
  RC_TRY(dev_array(e, t.dev, &t.d_bins, th.bins.data(), th.bins.size() * sizeof(RowBin), 0));
  RC_TRY(dev_array(e, t.dev, &t.d_chunks, th.chunks.data(), th.chunks.size() * sizeof(TileChunk), 0));
  if (!th.vdict.empty()) {
    t.n_vdict = (int)th.vdict.size();
    t.n_vdict_used = th.vdict_used;
    t.code_bits = th.code_bits;
    t.skip_minplus = true;   // (known from the dictionary alone; raw values would need a pass over the matrix: not skipped)
    for (int k = 0; k < th.vdict_used; k++) t.skip_minplus = t.skip_minplus && (th.vdict[(size_t)k] & 0x7FFFFFFFu) < 0x73000000u;   // |a| < 2^103
    RC_TRY(plan_array(e, m, &t.d_tcode, td.tcode, td.n_tcode, th.tcode, SLACK_TCODE));
    RC_TRY(dev_array(e, t.dev, &t.d_vdict, th.vdict.data(), th.vdict.size() * 4, 0));
  } else {
    RC_TRY(plan_array(e, m, &t.d_tval, td.tval, td.n_tval, th.tval, SLACK_WIDE));
  }
  RC_TRY(plan_array(e, m, &t.d_tcol, td.tcol, td.n_tcol, th.tcol, SLACK_WIDE));
  RC_TRY(plan_array(e, m, &t.d_gdest, td.gdest, td.n_gdest, th.gdest, SLACK_WIDE));
  RC_TRY(plan_array(e, m, &t.d_gblk, td.gblk, td.n_gblk, th.gblk, SLACK_WIDE));
  RC_TRY(plan_array(e, m, &t.d_ptab, td.ptab, td.n_ptab, th.ptab, SLACK_WIDE));
  RC_TRY(plan_array(e, m, &t.d_ptile, td.ptile, td.n_ptab, th.ptile, SLACK_WIDE));
  t.n_pieces = (int64_t)(m->built_on_device ? td.n_ptab : th.ptab.size());
  // dead pieces (launches of a semiring with absorbing words): the marked copy of ptab, the tiles' live words (all live until a launch says otherwise)
  RC_TRY(dev_array(e, t.dev, &t.d_ptab_live, nullptr, (size_t)t.n_pieces * 4, SLACK_WIDE));
  const size_t ct = (size_t)std::max<int64_t>(1, (m->cols + t.tcols - 1) / t.tcols);
  RC_TRY(dev_array(e, t.dev, &t.d_tile_live, nullptr, ct * 4, 0));
  HIP_TRY(e, hipMemsetD32Async((hipDeviceptr_t)t.d_tile_live, 1, ct, e->stream));
  RC_TRY(plan_array(e, m, &t.d_pslot, td.pslot, td.n_pslot, th.pslot, SLACK_WIDE));
  RC_TRY(plan_array(e, m, &t.d_obase, td.obase, td.n_obase, th.obase, SLACK_WIDE));
  if (t.tcols != TCOLS) RC_TRY(plan_array(e, m, &t.d_fmask, td.fmask, td.n_fmask, th.fmask, SLACK_WIDE));
  RC_TRY(dev_array(e, t.dev, &t.d_P, nullptr, (size_t)std::max<int64_t>(t.p_len, 4) * 4, 16));
  RC_TRY(plan_array(e, m, (uint32_t **)&t.d_lrp, td.lrp, td.n_lrp, th.lrp, 16));   // (+16: see plan_gpu.hip)
  if (t.n_tlong) {
    RC_TRY(dev_array(e, t.dev, &t.d_tlong, th.heavy.data(), th.heavy.size() * sizeof(LongRow), 0));
    RC_TRY(dev_array(e, t.dev, &t.d_tpartial, nullptr, (size_t)th.n_partials * 4, 16));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream)); // host vectors die with the caller's th
  lap("hipMalloc + H2D of the plan");
  return SH_OK;
}

// The CSR-stream layout: the CSR arrays (uploaded unless a device builder had them already) and the block schedule.
static int upload_stream_layout(sh_engine *e, sh_csr *m, const HostCsr &h) {
  StreamLayout &s = m->stream;
  std::vector<int32_t> pairs;
  std::vector<LongSeg> segs;
  std::vector<LongRow> longs;
  build_schedule(h.rows, h.row_ptr, pairs, segs, longs);
  s.n_stream = (int32_t)(pairs.size() / 2);
  s.n_segs = (int32_t)segs.size();
  s.n_long = (int32_t)longs.size();
  RC_TRY(upload_csr_arrays(e, m, h));
  // The kernel reads blk_row[b] and blk_row[b+1]; with long rows in between the
  // blocks are not contiguous, so upload the pair list and index it as 2*b.
  RC_TRY(dev_array(e, s.dev, &s.d_blk_row, pairs.data(), pairs.size() * 4, 8));
  if (s.n_segs) {
    RC_TRY(dev_array(e, s.dev, &s.d_segs, segs.data(), segs.size() * sizeof(LongSeg), 0));
    RC_TRY(dev_array(e, s.dev, &s.d_long, longs.data(), longs.size() * sizeof(LongRow), 0));
    RC_TRY(dev_array(e, s.dev, &s.d_partial, nullptr, segs.size() * 4, 0));
    RC_TRY(dev_array(e, s.dev, &s.d_partial_multi, nullptr, segs.size() * 4 * SPMM_MAX_WIDTH, 0));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream)); // host vectors die at return
  return SH_OK;
}

struct CsrDeleter {   // (a matrix given up half-way: the copies enqueued from host vectors have to land first)
  sh_engine *e;
  void operator()(sh_csr *m) const { free_handle(e, m); }
};

int sh_csr_upload_ex(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr,
                     const int32_t *col_idx, const void *val, const sh_plan_options *opt_p, sh_csr **out) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  if (!e || !out || rows < 0 || cols < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!col_idx || !val)))
    return fail(e, SH_EINVAL, "sh_csr_upload: bad argument");
  if (rows > INT32_MAX - 1 || cols > INT32_MAX || nnz > INT32_MAX - 8)
    return fail(e, SH_EINVAL, "sh_csr_upload: sizes exceed int32 indexing (shard the matrix)");
  if (row_ptr[0] != 0 || row_ptr[rows] != nnz)
    return fail(e, SH_ESHAPE, "sh_csr_upload: row_ptr[0]=%d row_ptr[rows]=%d, nnz=%lld", row_ptr[0],
                row_ptr[rows], (long long)nnz);
  *out = nullptr;
  HIP_TRY(e, hipSetDevice(e->device));
  std::unique_ptr<sh_csr, CsrDeleter> m(new (std::nothrow) sh_csr(), CsrDeleter{e});
  if (!m)
    return fail(e, SH_ENOMEM, "out of host memory");
  m->rows = rows; m->cols = cols; m->nnz = nnz;
  for (int64_t r = 0; r < rows; r++)
    if (row_ptr[r + 1] < row_ptr[r])
      return fail(e, SH_ESHAPE, "sh_csr_upload: row_ptr not monotone at row %lld", (long long)r);
  const HostCsr h{rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val};
  const bool device_build = opt.build == 2 || (opt.build == 0 && nnz >= DEVICE_BUILD_MIN_NNZ);

  // The (or,and) semiring on bits, when asked for (or_and_bits: 1 = beside the ordinary plan, 2 = instead of it: a BFS
  // harness never launches another semiring on its matrix)
  if (opt.or_and_bits > 0 && nnz > 0)
    RC_TRY(build_bits_layout(e, m.get(), h, opt, device_build));
  if (m->bits_only && m->bits.d_bits_items) {
    drop_stream_layout(e, m.get());
    m->plan = PLAN_STREAM;
    *out = m.release();
    return SH_OK;
  }
  m->bits_only = false;
  // The tiled plan first: when it is chosen and nothing asks for a timing of both plans, the CSR arrays
  // (8 B per entry) are neither uploaded nor kept -- the tiled kernels read their own layout only.
  TiledHost th;
  TiledDevArrays td;   // the big arrays when the layout was built on the device
  struct TdGuard { TiledDevArrays &t; ~TdGuard() { t.release(); } } td_guard{td};   // (whatever was not adopted below)
  lap(nullptr);
  const bool bits_on_device = m->built_on_device;
  m->built_on_device = false;   // (from here on: the tiled layout)
  bool tiled = false;
  RC_TRY(build_tiled_layout(e, m.get(), h, opt, device_build, th, td, &tiled));
  // (only worth timing when the bins touch few of the column tiles, i.e. the columns are local: with
  // scattered columns -- every bin has a piece in nearly every tile -- plan A is several times slower)
  const bool tune = tiled && opt.plan == 0 && opt.autotune && th.tile_fill < 0.5;
  m->plan = tiled ? PLAN_TILED : PLAN_STREAM;
  // The CSR arrays (8 B per entry) stay on the device only for plan A, or while both plans are timed.
  if (!tiled || tune)
    RC_TRY(upload_stream_layout(e, m.get(), h));
  else
    drop_stream_layout(e, m.get());
  if (tiled)
    RC_TRY(upload_tiled_layout(e, m.get(), opt, th, td));
  if (tune)
    autotune_plan(e, m.get());   // drops the layout of the plan that lost
  {
    // placements of the big arrays to try: the option, else six for a matrix whose product array has >= 2^22 words.
    // Eight fresh processes per setting, one box each time (profiles/r03_ab_placement_tries*.log): 1 / 3 / 6 tries
    // 0.4476 / 0.4384 / 0.4331 ms; on another box 1 / 6 / 12 / 24 tries 0.4456 / 0.4413 / 0.4391 / 0.4417 (means): a trial
    // predicts the steady state of the caller's loop (other x and out vectors) only in part, and past six nothing is gained.
    const int tries = opt.placement_tries > 0 ? opt.placement_tries : (m->plan == PLAN_TILED && m->tiled.p_len >= ((int64_t)1 << 22) ? 6 : 1);
    tune_placement(e, m.get(), tries);
  }
  if (bits_on_device && !tiled) m->built_on_device = true;   // (a matrix whose only device-built layout is the bit-blocked one)
  *out = m.release();
  return SH_OK;
}

int sh_csr_free(sh_engine *e, sh_csr *m) { return free_handle(e, m); }

int sh_csr_builder(const sh_csr *m, int32_t *where, char *note, int64_t cap) {
  if (!m)
    return SH_EINVAL;
  if (where) *where = m->built_on_device ? 1 : 0;
  if (note && cap > 0) snprintf(note, (size_t)cap, "%s", m->build_note.c_str());
  return SH_OK;
}

int sh_csr_placement(const sh_csr *m, int32_t *tries, float *first_ms, float *kept_ms) {
  if (!m)
    return SH_EINVAL;
  if (tries) *tries = m->placement_tries;
  if (first_ms) *first_ms = m->placement_ms[0];
  if (kept_ms) *kept_ms = m->placement_ms[1];
  return SH_OK;
}

int sh_csr_dims(const sh_csr *m, int64_t *rows, int64_t *cols, int64_t *nnz) {
  if (!m)
    return SH_EINVAL;
  if (rows) *rows = m->rows;
  if (cols) *cols = m->cols;
  if (nnz) *nnz = m->nnz;
  return SH_OK;
}

int sh_csr_algorithmic_bytes(const sh_csr *m, int reads_y, uint64_t *bytes) {
  if (!m || !bytes)
    return SH_EINVAL;
  *bytes = 8ull * m->nnz + 4ull * (m->rows + 1) + 4ull * m->cols + 4ull * m->rows +
           (reads_y ? 4ull * m->rows : 0ull);
  return SH_OK;
}

int sh_csr_plan(const sh_csr *m, int32_t *plan, uint64_t *streamed_bytes) {
  if (!m)
    return SH_EINVAL;
  if (plan) *plan = m->bits_only ? 2 : m->plan;
  if (streamed_bytes && m->bits_only) {   // 4 B per entry, the x bitmap and the partial result bitmaps written and read once, the vectors
    *streamed_bytes = 4ull * (uint64_t)m->bits.bits_entries + 2ull * (uint64_t)m->bits.n_bits_items * (BITS_BR / 8) +
                      (uint64_t)m->bits.n_bits_items * (BITS_BC / 8) + 4ull * m->cols + 8ull * m->rows;
    return SH_OK;
  }
  if (streamed_bytes) {
    const uint64_t vec = 4ull * (m->rows + 1) + 4ull * m->cols + 4ull * m->rows;
    *streamed_bytes = (m->plan == PLAN_TILED)
                          ? (m->tiled.n_vdict ? 2ull : 6ull) * m->tiled.stream_len + (m->tiled.n_vdict ? (uint64_t)m->tiled.stream_len * m->tiled.code_bits / 8 : 0ull) + (uint64_t)(m->tiled.stream_len - m->tiled.light_len) / 4 /* gdest: 4 B per 16-entry strip */ +
                                (uint64_t)m->tiled.light_len / 64 /* obase: 4 B per 64 groups */ + (m->tiled.d_fmask ? (uint64_t)m->tiled.light_len / 32 /* fmask: 8 B */ : 0ull) +
                                4ull * m->tiled.p_len /* P written */ + 6ull * m->tiled.p_len + m->tiled.p_len / 6 /* phase 2: P, slot; piece tables ~0.14 B per product */ +
                                vec /* x once: a tile is re-staged per phase-1 workgroup, but out of its XCD's L2 */
                          : 8ull * m->nnz + vec;
  }
  return SH_OK;
}

int sh_csr_describe(const sh_csr *m, char *buf, size_t buflen) {
  if (!m || !buf || buflen == 0)
    return SH_EINVAL;
  if (m->plan == PLAN_TILED) {
    const TiledLayout &t = m->tiled;
    describe_tiled(buf, buflen, m->cols, t.tcols, t.n_vdict, t.code_bits, t.n_vdict_used, t.n_chunks, t.n_bins, t.n_tlong, t.stream_len,
                   t.light_entries, t.p_len, t.fold != 0);
  } else if (m->bits_only) {
    snprintf(buf, buflen, "bits-only");
  } else {
    snprintf(buf, buflen, "stream values=raw blocks=%d long_rows=%d segments=%d", m->stream.n_stream, m->stream.n_long, m->stream.n_segs);
  }
  if (m->tuned) {
    const size_t len = strlen(buf);
    snprintf(buf + len, buflen - len, " tuned(stream=%.3fms,tiled=%.3fms)", m->tuned_ms[0], m->tuned_ms[1]);
  }
  {
    const size_t len = strlen(buf);
    if (m->bits.d_bits_items)
      snprintf(buf + len, buflen - len, " or_and=bits(items=%d,entries=%.1fM%s)", m->bits.n_bits_items, m->bits.bits_entries / 1e6, m->bits_only ? ",only" : "");
    const size_t len2 = strlen(buf);
    snprintf(buf + len2, buflen - len2, " device=%.3fGB", (double)m->device_bytes() / 1e9);
  }
  return SH_OK;
}

int sh_csr_footprint(const sh_csr *m, uint64_t *device_bytes) {
  if (!m || !device_bytes)
    return SH_EINVAL;
  *device_bytes = (uint64_t)m->device_bytes();
  return SH_OK;
}

// ---------------------------------------------------------------- vectors
int sh_vec_alloc(sh_engine *e, int64_t n, sh_vec **out) {
  if (!e || !out || n < 0)
    return fail(e, SH_EINVAL, "sh_vec_alloc: bad argument");
  *out = nullptr;
  HIP_TRY(e, hipSetDevice(e->device));
  sh_vec *v = new (std::nothrow) sh_vec();
  if (!v)
    return fail(e, SH_ENOMEM, "out of host memory");
  hipError_t r = hipMalloc(&v->d, (n > 0 ? n : 1) * 4);
  if (r != hipSuccess) {
    delete v;
    return fail(e, SH_ENOMEM, "hipMalloc(%lld B) failed: %s", (long long)n * 4, hipGetErrorString(r));
  }
  v->n = n;
  v->owned = true;
  *out = v;
  return SH_OK;
}

int sh_vec_wrap(sh_engine *e, void *device_ptr, int64_t n, sh_vec **out) {
  if (!e || !out || n < 0 || (!device_ptr && n > 0))
    return fail(e, SH_EINVAL, "sh_vec_wrap: bad argument");
  sh_vec *v = new (std::nothrow) sh_vec();
  if (!v)
    return fail(e, SH_ENOMEM, "out of host memory");
  v->d = device_ptr;
  v->n = n;
  v->owned = false;
  *out = v;
  return SH_OK;
}

int sh_vec_free(sh_engine *e, sh_vec *v) {
  if (!v)
    return SH_OK;
  if (v->owned && v->d) {
    if (e) {
      (void)hipSetDevice(e->device);
      (void)hipStreamSynchronize(e->stream);
    }
    (void)hipFree(v->d);
  }
  delete v;
  return SH_OK;
}

int sh_vec_upload(sh_engine *e, sh_vec *v, const void *host, int64_t n) {
  if (!e || !v || (!host && n > 0) || n < 0)
    return fail(e, SH_EINVAL, "sh_vec_upload: bad argument");
  if (n > v->n)
    return fail(e, SH_ESHAPE, "sh_vec_upload: %lld elements into a vector of %lld", (long long)n, (long long)v->n);
  HIP_TRY(e, hipMemcpyAsync(v->d, host, n * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return SH_OK;
}

int sh_vec_download(sh_engine *e, const sh_vec *v, void *host, int64_t n) {
  if (!e || !v || (!host && n > 0) || n < 0)
    return fail(e, SH_EINVAL, "sh_vec_download: bad argument");
  if (n > v->n)
    return fail(e, SH_ESHAPE, "sh_vec_download: %lld elements from a vector of %lld", (long long)n, (long long)v->n);
  HIP_TRY(e, hipMemcpyAsync(host, v->d, n * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return SH_OK;
}

int sh_vec_fill(sh_engine *e, sh_vec *v, uint32_t pattern32) {
  if (!e || !v)
    return fail(e, SH_EINVAL, "sh_vec_fill: bad argument");
  if (v->n > 0)
    HIP_TRY(e, hipMemsetD32Async((hipDeviceptr_t)v->d, (int)pattern32, v->n, e->stream));
  return SH_OK;
}

int sh_vec_copy(sh_engine *e, sh_vec *dst, const sh_vec *src) {
  if (!e || !dst || !src)
    return fail(e, SH_EINVAL, "sh_vec_copy: bad argument");
  if (dst->n != src->n)
    return fail(e, SH_ESHAPE, "sh_vec_copy: length mismatch");
  if (src->n > 0)
    HIP_TRY(e, hipMemcpyAsync(dst->d, src->d, src->n * 4, hipMemcpyDeviceToDevice, e->stream));
  return SH_OK;
}

int64_t sh_vec_len(const sh_vec *v) { return v ? v->n : -1; }
void *sh_vec_device_ptr(const sh_vec *v) { return v ? v->d : nullptr; }

} // extern "C"

// ---------------------------------------------------------------- launches
#ifdef SH_STATS
#include "stats_dump.h"
#endif

// The (or,and) semiring on bits: x -> bitmap, blocks -> partial result bitmaps, rows
template <class SR>
static int launch_bits_layout(sh_engine *e, const sh_csr *A, const sh_vec *x, const sh_vec *y, typename SR::T alpha, typename SR::T beta,
                              sh_vec *out, StepDev st) {
  const BitsLayout &b = A->bits;
  const uint32_t *yp = y ? (const uint32_t *)y->d : nullptr;
  const int64_t words32 = (int64_t)b.bits_ct * (BITS_BC / 32);
  hipLaunchKernelGGL(bits_pack_x, dim3((unsigned)((words32 * 8 + 255) / 256)), dim3(256), 0, e->stream, (const uint32_t *)x->d,
                     (int32_t)A->cols, (uint32_t *)b.d_xbits, words32, st.gate);
  HIP_TRY(e, hipGetLastError());
  if (b.n_bits_items > 0) {
    hipLaunchKernelGGL(bits_blocks, dim3((unsigned)b.n_bits_items), dim3(BITS_TBS), 0, e->stream, b.d_bits_items,
                       b.d_bits_ent, b.d_bits_sub, (const uint32_t *)b.d_xbits, b.d_bits_partial, st.gate);
    HIP_TRY(e, hipGetLastError());
  }
  if (A->rows > 0) {
    hipLaunchKernelGGL(bits_finish, dim3((unsigned)((A->rows + BITS_FIN_ROWS - 1) / BITS_FIN_ROWS)), dim3(256), 0, e->stream, b.d_bits_rr0,
                       b.d_bits_partial, (int32_t)A->rows, yp, alpha, beta, y ? 1 : 0, (uint32_t *)out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (st.expected) {
    hipLaunchKernelGGL(report_all_pieces, dim3(1), dim3(64), 0, e->stream, st);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

// Phase 1 of the tiled plan for one way of storing the values: CODE 0 raw words (d_tval), 1 / 2 / 3 dictionary codes of
// 8 / 4 / 16 bits (d_tcode, d_vdict), and for the layout's tile width (WIDE: TCOLS_WIDE columns, fold flags in d_fmask).
template <class SR, int CODE, bool WIDE>
static void launch_phase1_as(sh_engine *e, const sh_csr *A, const sh_vec *x, StepDev st, int32_t skip_dead, uint32_t *tile_live) {
  const TiledLayout &t = A->tiled;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_tiled_phase1<SR, CODE, WIDE>), dim3((unsigned)t.n_chunks), dim3(TBS), 0, e->stream,
                     (const TileChunk *)t.d_chunks, CODE ? (const void *)t.d_tcode : (const void *)t.d_tval,
                     CODE ? (const uint32_t *)t.d_vdict : (const uint32_t *)nullptr, t.d_tcol, t.d_gdest, t.d_obase, (const uint64_t *)t.d_fmask,
                     (const uint32_t *)x->d, (int32_t)A->cols, t.d_P, t.d_tpartial, st.gate, skip_dead, tile_live);
}
template <class SR, int CODE>
static int launch_phase1(sh_engine *e, const sh_csr *A, const sh_vec *x, StepDev st, int32_t skip_dead, uint32_t *tile_live) {
  const TiledLayout &t = A->tiled;
  if (t.tcols == TCOLS) { launch_phase1_as<SR, CODE, false>(e, A, x, st, skip_dead, tile_live); return SH_OK; }
  // (two-byte codes have no wide kernel: their dictionary takes the LDS, and the builders keep such a layout narrow)
  if constexpr (CODE != 3) {
    if (t.tcols == TCOLS_WIDE && t.d_fmask) { launch_phase1_as<SR, CODE, true>(e, A, x, st, skip_dead, tile_live); return SH_OK; }
  }
  return SH_EINVAL;
}

template <class SR>
static int launch_tiled(sh_engine *e, const sh_csr *A, const sh_vec *x, const sh_vec *y, typename SR::T alpha, typename SR::T beta,
                        sh_vec *out, StepDev st) {
  const TiledLayout &t = A->tiled;
  const uint32_t *yp = y ? (const uint32_t *)y->d : nullptr;
#ifdef SH_STATS
  stats_before_tiled(e);
#endif
  // tiles whose x words are all absorbing are not streamed (semiring.hip.h); (min,+) needs every |value| < 2^103
  const int32_t skip_dead = SR::id == 1 ? (t.skip_minplus ? 1 : 0) : 1;
  // ... and their products are neither written by phase 1 nor read by phase 2: phase 1 leaves a live word per tile,
  // tiled_mark_dead turns it into a copy of the piece table whose dead pieces point at one group of identity
  // words, phase 2 reads the pieces through that copy (semirings with absorbing words only)
  const bool mark_dead = SR::has_absorbing && skip_dead && t.n_bins > 0 && t.n_pieces > 0;
  uint32_t *tile_live = mark_dead ? t.d_tile_live : nullptr;
  if (t.n_chunks > 0) {
    int rc1;
    if (!t.n_vdict) rc1 = launch_phase1<SR, 0>(e, A, x, st, skip_dead, tile_live);
    else if (t.code_bits == 16) rc1 = launch_phase1<SR, 3>(e, A, x, st, skip_dead, tile_live);
    else if (t.code_bits == 4) rc1 = launch_phase1<SR, 2>(e, A, x, st, skip_dead, tile_live);
    else rc1 = launch_phase1<SR, 1>(e, A, x, st, skip_dead, tile_live);
    if (rc1 != SH_OK) return rc1;
    HIP_TRY(e, hipGetLastError());
  }
  if (mark_dead) {
    const uint32_t ident = SR::identity_bits;
    hipLaunchKernelGGL(tiled_mark_dead, dim3((unsigned)((t.n_pieces + 255) / 256)), dim3(256), 0, e->stream, t.d_ptab, t.d_ptile,
                       (const uint32_t *)t.d_tile_live, t.d_ptab_live, t.n_pieces, t.d_P + std::max<int64_t>(t.p_len, 4), ident, st.gate);
    HIP_TRY(e, hipGetLastError());
  }
  // phase 2; its reducer waves also add up the heavy rows' partials while the loaders fill the first bin
  if (t.n_bins > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_tiled_phase2s<SR>), dim3(std::min(t.n_bins, e->n_cus)), dim3(P2S_BS), 0,
                       e->stream, t.d_bins, t.n_bins, t.d_lrp, t.d_P, (int32_t)(std::max<int64_t>(t.p_len, 4) / 4 - 1), t.d_pslot,
                       (const uint4 *)t.d_gblk, mark_dead ? t.d_ptab_live : t.d_ptab, t.d_tlong, t.n_tlong, t.d_tpartial, yp, alpha, beta, y ? 1 : 0,
                       (uint32_t *)out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
#ifdef SH_STATS
  stats_after_tiled(e, t.n_bins, t.n_chunks);
#endif
  if (t.n_bins == 0 && t.n_tlong > 0) {   // every row is heavy: no phase 2 to host the sums
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_heavy_fixup<SR>), dim3(t.n_tlong), dim3(HFIX_BS), 0, e->stream, t.d_tlong,
                       t.d_tpartial, yp, alpha, beta, y ? 1 : 0, (uint32_t *)out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (st.expected && t.n_bins == 0) {      // nobody reported: one arrival per piece behind everything
    hipLaunchKernelGGL(report_all_pieces, dim3(1), dim3(64), 0, e->stream, st);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

template <class SR>
static int launch_stream(sh_engine *e, const sh_csr *A, const sh_vec *x, const sh_vec *y, typename SR::T alpha, typename SR::T beta,
                         sh_vec *out, StepDev st) {
  const StreamLayout &s = A->stream;
  const uint32_t *yp = y ? (const uint32_t *)y->d : nullptr;
  CsrDev dev{s.d_row_ptr, s.d_col, s.d_val, (int32_t)A->rows, (int32_t)A->cols};
  const int grid = s.n_stream + s.n_segs;
  if (grid > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_csr_kernel<SR>), dim3(grid), dim3(BS), 0, e->stream, dev,
                       (const uint32_t *)x->d, yp, alpha, beta, y ? 1 : 0, (uint32_t *)out->d, s.d_blk_row, s.n_stream, s.d_segs,
                       s.d_partial, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (s.n_long > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmv_long_fixup<SR>), dim3((s.n_long + 63) / 64), dim3(64), 0,
                       e->stream, s.d_long, s.n_long, s.d_partial, yp, alpha, beta, y ? 1 : 0, (uint32_t *)out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (st.expected) {   // the CSR-stream kernels do not report pieces: one arrival per piece behind them
    hipLaunchKernelGGL(report_all_pieces, dim3(1), dim3(64), 0, e->stream, st);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

// One launch of the layout that serves the semiring: the bit-blocked one for (or,and) where the matrix has it, else the
// matrix's plan.  They get y where the epilogue reads it, else NULL.
template <class SR>
static int launch_spmv(sh_engine *e, const sh_csr *A, const sh_vec *x, const sh_vec *y,
                       const void *alpha_p, const void *beta_p, sh_vec *out, StepDev st) {
  using T = typename SR::T;
  T alpha, beta;
  memcpy(&alpha, alpha_p, 4);
  memcpy(&beta, beta_p, 4);
  const bool use_y = SR::reads_y(beta);
  if (use_y && !y)
    return fail(e, SH_EINVAL, "sh_spmv: y is NULL but the epilogue reads it (beta != 0 or min-plus)");
  if (use_y && y->n < A->rows)
    return fail(e, SH_ESHAPE, "sh_spmv: y has %lld elements, matrix has %lld rows", (long long)y->n, (long long)A->rows);
  if (!use_y) y = nullptr;
  if constexpr (std::is_same<SR, OrAndI32>::value)
    if (A->bits.d_bits_items) return launch_bits_layout<SR>(e, A, x, y, alpha, beta, out, st);
  if (A->bits_only)
    return fail(e, SH_EINVAL, "this matrix was uploaded with or_and_bits = 2: it serves SH_OR_AND_I32 launches only");
  if (A->plan == PLAN_TILED)
    return launch_tiled<SR>(e, A, x, y, alpha, beta, out, st);
  return launch_stream<SR>(e, A, x, y, alpha, beta, out, st);
}

// Whether the epilogue of the semiring reads y (any other value of sr: refused by the dispatch).
static bool reads_y(sh_semiring sr, const void *beta_p) {
  float bf;
  int32_t bi;
  memcpy(&bf, beta_p, 4);
  memcpy(&bi, beta_p, 4);
  switch (sr) {
  case SH_PLUS_TIMES_F32: return PlusTimesF32::reads_y(bf);
  case SH_MIN_PLUS_F32: return MinPlusF32::reads_y(bf);
  case SH_OR_AND_I32: return OrAndI32::reads_y(bi);
  default: return MaxMinI32::reads_y(bi);
  }
}

// The state of a matrix's piece reports, made by its first sh_spmv_step_pieces launch: whole, or not at all.
static int open_piece_report(sh_engine *e, sh_csr *A) {
  std::unique_ptr<PieceReport> p(new (std::nothrow) PieceReport());
  if (!p)
    return fail(e, SH_ENOMEM, "out of host memory");
  HIP_TRY(e, p->dev.alloc_exact(&p->d_done, MAX_PIECES * 4));
  HIP_TRY(e, p->dev.alloc_exact(&p->d_pcs, sizeof(PieceDev)));
  HIP_TRY(e, hipHostMalloc((void **)&p->h_done, 64, hipHostMallocDefault));
  memset(p->h_done, 0, 64);
  HIP_TRY(e, hipMemsetAsync(p->d_done, 0, MAX_PIECES * 4, e->stream));
  A->pieces = std::move(p);
  return SH_OK;
}

static int check_operands(sh_engine *e, const sh_csr *A, const sh_vec *x, const void *alpha,
                          const void *beta, const sh_vec *out, const char *who) {
  if (!e || !A || !x || !alpha || !beta || !out)
    return fail(e, SH_EINVAL, "%s: NULL argument", who);
  if (x->n < A->cols)
    return fail(e, SH_ESHAPE, "%s: x has %lld elements, matrix has %lld columns", who, (long long)x->n, (long long)A->cols);
  if (out->n < A->rows)
    return fail(e, SH_ESHAPE, "%s: out has %lld elements, matrix has %lld rows", who, (long long)out->n, (long long)A->rows);
  if (out->d == x->d && A->rows > 0)
    return fail(e, SH_EINVAL, "%s: out must not alias x", who);
  return SH_OK;
}

static int dispatch(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x, const sh_vec *y,
                    const void *alpha, const void *beta, sh_vec *out, StepDev st) {
  switch (sr) {
  case SH_PLUS_TIMES_F32: return launch_spmv<PlusTimesF32>(e, A, x, y, alpha, beta, out, st);
  case SH_MIN_PLUS_F32: return launch_spmv<MinPlusF32>(e, A, x, y, alpha, beta, out, st);
  case SH_OR_AND_I32: return launch_spmv<OrAndI32>(e, A, x, y, alpha, beta, out, st);
  case SH_MAX_MIN_I32: return launch_spmv<MaxMinI32>(e, A, x, y, alpha, beta, out, st);
  default: return fail(e, SH_EINVAL, "unknown semiring %d", (int)sr);
  }
}

// ---- the dense iteration loops ---------------------------------------------------------------------------------------
static hipError_t ms_between(hipEvent_t a, hipEvent_t b, uint64_t *ns) {
  float ms = 0.f;
  const hipError_t r = hipEventElapsedTime(&ms, a, b);
  *ns = (uint64_t)((double)ms * 1e6);
  return r;
}

// The vectors of an iteration: a launch reads `in` (and `y`) and writes `out`; one that swaps hands its output to the next.
struct PingPong {
  sh_vec *in, *out;
  const sh_vec *y;
  uint32_t swapped = 0;   // bit k: launch k of the batch under way exchanged the buffers
  void swap(int k) {
    std::swap(in, out);   // std::swap(input, output), app/sssp.cpp:143
    y = in;               // setGlobalArg(3, input_mem_ptr), :150
    swapped |= 1u << k;
  }
  // The batch is over.  Its launches from `ran` on returned at their gate and wrote nothing: the result is what launch
  // ran - 1 produced, so the exchanges that were enqueued for them are taken back.
  void end_batch(int ran) {
    if (__builtin_popcount(swapped >> ran) % 2) std::swap(in, out);
    y = in;
    swapped = 0;
  }
  int hand_back(sh_engine *e, sh_vec *x, size_t bytes) const {   // the final vector may live in the scratch vector
    if (in == x)
      return SH_OK;
    HIP_TRY(e, hipMemcpyAsync(x->d, in->d, bytes, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return SH_OK;
  }
};

struct Readback { void *host; const void *dev; size_t bytes; };   // what a batch copies back before the host joins in
struct DenseRun { int32_t launches = 0; bool over = false; uint64_t total_ns = 0; };

// The loop of sh_iterate, sh_iterate_multi, sh_bits_iterate and sh_iterate_frontier: up to BATCH gated launches are
// enqueued ahead of the host, which joins in once per batch (DESIGN.md "The dense batch loop").  Per batch: begin()
// clears the state the launches write; enqueue(launch, k, pp, &swaps) enqueues launch `launch` as number k of the batch
// on pp.in / pp.y / pp.out and clears `swaps` if it leaves its result in pp.in; `rb` is copied back and the stream joined;
// settle(first, nb, &ran, &over) reads it: how many of the nb launches ran, whether the iteration is over, and the
// caller's per-launch outputs of launches first .. first + ran - 1.  The loop owns the events, the time of every launch
// that ran (ns_per_launch may be NULL), the buffers of the launches that did not, and the cap.
template <int BATCH, class Begin, class Enqueue, class Settle>
static int run_dense_batches(sh_engine *e, PingPong &pp, int32_t cap, Readback rb, uint64_t *ns_per_launch, DenseRun *run,
                             Begin begin, Enqueue enqueue, Settle settle) {
  hipEvent_t *ev = e->dense.ev;
  static_assert(BATCH <= 8, "one event per launch of a batch, and one bit of PingPong::swapped");
  if (!ev[0])
    for (auto &v : e->dense.ev) HIP_TRY(e, hipEventCreate(&v));
  int32_t it = 0;
  bool over = false;
  while (!over && it < cap) {
    const int nb = std::min<int32_t>(BATCH, cap - it);
    RC_TRY(begin());
    HIP_TRY(e, hipEventRecord(ev[0], e->stream));
    for (int k = 0; k < nb; k++) {
      bool swaps = true;
      RC_TRY(enqueue(it + k, k, pp, &swaps));
      HIP_TRY(e, hipEventRecord(ev[k + 1], e->stream));
      if (swaps) pp.swap(k);
    }
    HIP_TRY(e, hipMemcpyAsync(rb.host, rb.dev, rb.bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    int ran = 0;
    RC_TRY(settle(it, nb, &ran, &over));
    for (int k = 0; k < ran; k++) {
      uint64_t ns = 0;
      HIP_TRY(e, ms_between(ev[k], ev[k + 1], &ns));
      if (ns_per_launch)
        ns_per_launch[it + k] = ns;
      run->total_ns += ns;
    }
    pp.end_batch(ran);
    it += ran;
  }
  run->launches = it;
  run->over = over;
  return SH_OK;
}

// sh_iterate_multi and sh_bits_iterate: the n columns (sources) of one vector converge each on its own.  `d` / `h` hold
// BATCH + 1 slots of SLOT words and `state_words` in all.  Slot k + 1 takes the flags of launch k of the batch, which
// launch k + 1 reads as its live mask; slot 0 carries those of the previous batch's last launch, and the first launch
// ever has no mask (NULL: everything is live).  launch(k, pp, flags, live) enqueues; flag(slot, j) reads column j's flag
// from a slot of `h`; extra(launch, k) takes whatever else launch k of the batch left behind slot BATCH.  A column's
// count = index of its first flag that stayed 0, plus one (the confirming launch included), or every launch made.
template <int SLOT, class W, class Launch, class Flag, class Extra>
static int iterate_slots(sh_engine *e, PingPong &pp, BatchWords<W> st, int state_words, int read_words, int n, int32_t max_iters,
                         int32_t *iters_of, int32_t *converged_of, uint64_t *ns_per_launch, DenseRun *run, Launch launch,
                         Flag flag, Extra extra) {
  constexpr int BATCH = 8;
  int n_live = n, last_slot = -1;   // slot of the latest launch that ran (-1: none yet)
  auto begin = [&]() -> int {
    if (last_slot > 0)
      HIP_TRY(e, hipMemcpyAsync(st.d, st.d + last_slot * SLOT, SLOT * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(e, hipMemsetAsync(st.d + SLOT, 0, (state_words - SLOT) * 4, e->stream));
    return SH_OK;
  };
  auto enqueue = [&](int32_t, int k, const PingPong &p, bool *) -> int {
    return launch(k, p, st.d + (k + 1) * SLOT, (k == 0 && last_slot < 0) ? nullptr : st.d + k * SLOT);
  };
  auto settle = [&](int32_t first, int nb, int *ran, bool *over) -> int {
    while (*ran < nb && n_live > 0) {   // every launch up to the first that left nothing live did run
      for (int j = 0; j < n; j++)
        if (!converged_of[j] && !flag(st.h + (*ran + 1) * SLOT, j)) {
          converged_of[j] = 1;
          iters_of[j] = first + *ran + 1;
          n_live--;
        }
      extra(first + *ran, *ran);
      ++*ran;
    }
    last_slot = *ran;
    *over = n_live == 0;
    return SH_OK;
  };
  RC_TRY(run_dense_batches<BATCH>(e, pp, max_iters, Readback{st.h, st.d, (size_t)read_words * 4}, ns_per_launch, run, begin, enqueue, settle));
  for (int j = 0; j < n; j++)
    if (!converged_of[j])
      iters_of[j] = run->launches;
  return SH_OK;
}

extern "C" {

int sh_spmv(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x, const sh_vec *y,
            const void *alpha, const void *beta, sh_vec *out, const sh_launch *launch,
            uint64_t *kernel_ns) {
  (void)launch;   // grid and workgroup size come from the matrix schedule (see header)
  int rc = check_operands(e, A, x, alpha, beta, out, "sh_spmv");
  if (rc)
    return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  StepDev st{nullptr, nullptr, 0, 0.0};
  if (kernel_ns)
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  rc = dispatch(e, sr, A, x, y, alpha, beta, out, st);
  if (rc)
    return rc;
  if (kernel_ns) {
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ns = (uint64_t)((double)ms * 1e6);
  }
  return SH_OK;
}

int sh_spmv_step(sh_engine *e, sh_semiring sr, const sh_csr *A, const sh_vec *x, const sh_vec *y,
                 const void *alpha, const void *beta, sh_vec *out, int64_t x_row_offset, double delta,
                 int32_t *changed_flag_device) {
  int rc = check_operands(e, A, x, alpha, beta, out, "sh_spmv_step");
  if (rc)
    return rc;
  if (x_row_offset < 0 || x_row_offset + A->rows > x->n)
    return fail(e, SH_ESHAPE, "sh_spmv_step: x_row_offset %lld + rows %lld exceeds x length %lld",
                (long long)x_row_offset, (long long)A->rows, (long long)x->n);
  HIP_TRY(e, hipSetDevice(e->device));
  StepDev st{changed_flag_device, (const uint32_t *)x->d, x_row_offset, delta};
  return dispatch(e, sr, A, x, y, alpha, beta, out, st);
}

int sh_spmv_step_pieces(sh_engine *e, sh_semiring sr, sh_csr *A, const sh_vec *x, const sh_vec *y,
                        const void *alpha, const void *beta, sh_vec *out, const sh_row_pieces *pc, double delta,
                        int32_t *changed_flag_device, uint32_t *round, const volatile uint32_t **done_words) {
  if (!e || !A || !x || !alpha || !beta || !out || !pc)
    return fail(e, SH_EINVAL, "sh_spmv_step_pieces: NULL argument");
  if (pc->n_pieces < 1 || pc->n_pieces > MAX_PIECES || pc->piece_rows < 1 ||
      (int64_t)pc->piece_rows * pc->n_pieces < A->rows)
    return fail(e, SH_EINVAL, "sh_spmv_step_pieces: %d pieces of %d rows do not cover %lld rows (at most %d pieces)",
                pc->n_pieces, pc->piece_rows, (long long)A->rows, MAX_PIECES);
  if (x->n < A->cols)
    return fail(e, SH_ESHAPE, "sh_spmv_step_pieces: x has %lld elements, matrix has %lld columns", (long long)x->n, (long long)A->cols);
  if (out->d == x->d && A->rows > 0)
    return fail(e, SH_EINVAL, "sh_spmv_step_pieces: out must not alias x");
  // A gated launch cannot report: behind a gate that reads 0 the tiled plan's phase 2 never arrives (the host words
  // would stay below *round for ever) while the other plans would report a round in which nothing was written.
  if (pc->report && pc->gate)
    return fail(e, SH_EINVAL, "sh_spmv_step_pieces: a gated launch cannot report its pieces (report != 0 with a gate)");
  // What the launch itself would refuse is refused here, before the round moves: a refused call leaves *round alone.
  if ((int)sr < SH_PLUS_TIMES_F32 || (int)sr > SH_MAX_MIN_I32)
    return fail(e, SH_EINVAL, "unknown semiring %d", (int)sr);
  if (reads_y(sr, beta) && !y)
    return fail(e, SH_EINVAL, "sh_spmv_step_pieces: y is NULL but the epilogue reads it (beta != 0 or min-plus)");
  if (A->bits_only && sr != SH_OR_AND_I32)
    return fail(e, SH_EINVAL, "this matrix was uploaded with or_and_bits = 2: it serves SH_OR_AND_I32 launches only");
  HIP_TRY(e, hipSetDevice(e->device));
  StepDev st{changed_flag_device, (const uint32_t *)x->d, 0, delta, pc->gate};
  PieceDev pd{};
  pd.n_pieces = pc->n_pieces;
  pd.piece_rows = pc->piece_rows;
  for (int c = 0; c < pc->n_pieces; c++) {
    const int64_t first = (int64_t)c * pc->piece_rows, rows_c = std::max<int64_t>(0, std::min<int64_t>(A->rows - first, pc->piece_rows));
    const int64_t at = pc->element_of_piece[c];
    if (at < 0 || at + rows_c > out->n || at + rows_c > x->n || (y && at + rows_c > y->n))
      return fail(e, SH_ESHAPE, "sh_spmv_step_pieces: piece %d (%lld rows at element %lld) does not fit the vectors", c, (long long)rows_c, (long long)at);
    pd.piece_delta[c] = at - first;
    // tiled plan: the piece is complete once every bin that starts below its last row + 1 is reduced
    pd.piece_bin_end[c] = (int32_t)(std::lower_bound(A->tiled.bin_r0.begin(), A->tiled.bin_r0.end(), (int32_t)std::min<int64_t>(first + pc->piece_rows, A->rows)) - A->tiled.bin_r0.begin());
  }
  if (pc->n_pieces > 0) pd.piece_bin_end[pc->n_pieces - 1] = (int32_t)A->tiled.bin_r0.size();
  if (!A->pieces)
    RC_TRY(open_piece_report(e, A));
  PieceReport &pr = *A->pieces;
  pd.done = pr.d_done;
  pd.done_host = pr.h_done;
  // the geometry goes to device memory once (an iteration loop brings the same one every time); a changed one is
  // copied behind the launches already enqueued on this stream, which keep reading the old bytes until then
  if (!pr.pcs_valid || memcmp(&pd, &pr.pcs_host, sizeof pd) != 0) {
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // (pcs_host is the copy's source: it must not change under a copy in flight)
    pr.pcs_host = pd;
    HIP_TRY(e, hipMemcpyAsync(pr.d_pcs, &pr.pcs_host, sizeof pd, hipMemcpyHostToDevice, e->stream));
    pr.pcs_valid = true;
  }
  st.pcs = pr.d_pcs;
  if (pc->report) {
    // arrivals per piece and launch: one per workgroup of phase 2, or the single one of report_all_pieces
    st.expected = (A->plan == PLAN_TILED && A->tiled.n_bins > 0 && !(sr == SH_OR_AND_I32 && A->bits.d_bits_items)) ? (uint32_t)std::min(A->tiled.n_bins, e->n_cus) : 1u;
    pr.round++;
    st.round = pr.round;
    pr.last_expected = st.expected;
    if (round) *round = pr.round;
    if (done_words) *done_words = pr.h_done;
  }
  // the epilogue reads y through the same row -> element mapping; an epilogue that does not read y gets none
  sh_vec yfull;
  if (y) { yfull = *y; yfull.owned = false; yfull.n = std::max<int64_t>(y->n, A->rows); }
  return dispatch(e, sr, A, x, y ? &yfull : nullptr, alpha, beta, out, st);
}

// Diagnosis of a piece report that does not arrive (the driver's wait timed out): the host words, what the latest
// reporting launch expects, and -- read through a stream of its own, so that a launch that never ends cannot block
// the question -- the device-side arrival counters (0xFFFFFFFF each when the copy itself did not finish in 2 s).
int sh_csr_piece_state(sh_engine *e, sh_csr *A, uint32_t *arrivals, uint32_t *host_words, uint32_t *expected, uint32_t *round) {
  if (!e || !A || !arrivals || !host_words)
    return fail(e, SH_EINVAL, "sh_csr_piece_state: NULL argument");
  const PieceReport *rep = A->pieces.get();   // (NULL: the matrix has not reported yet)
  if (expected) *expected = rep ? rep->last_expected : 0u;
  if (round) *round = rep ? rep->round : 0u;
  for (int c = 0; c < MAX_PIECES; c++) { arrivals[c] = 0xFFFFFFFFu; host_words[c] = rep ? ((volatile uint32_t *)rep->h_done)[c] : 0u; }
  if (!rep)
    return SH_OK;
  const PieceReport &pr = *rep;
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t side;
  HIP_TRY(e, hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  // (h_done is 16 words of pinned host memory: the upper 8 receive the counters)
  if (hipMemcpyAsync(pr.h_done + MAX_PIECES, pr.d_done, MAX_PIECES * 4, hipMemcpyDeviceToHost, side) == hipSuccess) {
    const auto t0 = std::chrono::steady_clock::now();
    bool ready = false;
    while (!(ready = hipStreamQuery(side) == hipSuccess) && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(2))
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (ready)
      for (int c = 0; c < MAX_PIECES; c++) arrivals[c] = ((volatile uint32_t *)pr.h_done)[MAX_PIECES + c];
  }
  (void)hipStreamDestroy(side);
  return SH_OK;
}

int sh_iterate(sh_engine *e, sh_semiring sr, const sh_csr *A, sh_vec *x, const sh_vec *y0,
               sh_vec *scratch, const void *alpha, const void *beta, double delta, int32_t max_iters,
               const sh_launch *launch, int32_t *iters, int32_t *converged, uint64_t *ns_per_iter,
               uint64_t *total_ns) {
  (void)launch;
  if (!e || !A || !x || !y0 || !scratch || !alpha || !beta || !iters || !converged || max_iters < 1)
    return fail(e, SH_EINVAL, "sh_iterate: bad argument");
  if (A->rows != A->cols)
    return fail(e, SH_ESHAPE, "sh_iterate: matrix must be square (inc/common.h:49-52)");
  if (x->n < A->rows || scratch->n < A->rows || y0->n < A->rows)
    return fail(e, SH_ESHAPE, "sh_iterate: vectors shorter than the matrix");
  if (scratch->d == x->d && A->rows > 0)
    return fail(e, SH_EINVAL, "sh_iterate: scratch must not alias x");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, e->dense.flags.open(64));
  const BatchWords<int32_t> &fl = e->dense.flags;
  // Iteration i carries the flag word of iteration i - 1 as its gate and returns at once when that flag stayed 0 (nothing
  // changed: the loop is over).  The launch count of the reference's do/while (app/sssp.cpp:112-153, confirming launch
  // included) = index of the first flag that stayed 0, plus one.
#ifndef SH_ITER_BATCH
#define SH_ITER_BATCH 8
#endif
  constexpr int ITER_BATCH = SH_ITER_BATCH;   // (1 = one host round trip per iteration, the round-1 loop: tools A/B builds)
  static_assert(ITER_BATCH <= 8, "the flags of a batch are read back into the first 8 words of the pinned copy");
  PingPong pp{x, scratch, y0};
  DenseRun run;
  auto begin = [&]() -> int {
    HIP_TRY(e, hipMemsetAsync(fl.d, 0, ITER_BATCH * 4, e->stream));
    return SH_OK;
  };
  auto enqueue = [&](int32_t, int k, const PingPong &p, bool *) -> int {
    StepDev st{fl.d + k, (const uint32_t *)p.in->d, 0, delta, k > 0 ? fl.d + (k - 1) : nullptr};
    return dispatch(e, sr, A, p.in, p.y, alpha, beta, p.out, st);
  };
  auto settle = [&](int32_t, int nb, int *ran, bool *over) -> int {
    *ran = nb;
    for (int k = 0; k < nb && !*over; k++)
      if (fl.h[k] == 0) { *ran = k + 1; *over = true; }
    return SH_OK;
  };
  RC_TRY(run_dense_batches<ITER_BATCH>(e, pp, max_iters, Readback{fl.h, fl.d, ITER_BATCH * 4}, ns_per_iter, &run, begin, enqueue, settle));
  RC_TRY(pp.hand_back(e, x, A->rows * 4));
  *iters = run.launches;
  *converged = run.over ? 1 : 0;
  if (total_ns)
    *total_ns = run.total_ns;
  return SH_OK;
}

} // extern "C"

// ---- K vectors per launch (multi.hip.h) -----------------------------------------------------------------------------
template <class SR, int K>
static int launch_spmm(sh_engine *e, const sh_csr *A, const sh_vec *X, const sh_vec *Y, const void *alpha_p,
                       const void *beta_p, sh_vec *Out, MultiStep st) {
  using T = typename SR::T;
  T alpha, beta;
  memcpy(&alpha, alpha_p, 4);
  memcpy(&beta, beta_p, 4);
  const bool use_y = SR::reads_y(beta);
  CsrDev dev{A->stream.d_row_ptr, A->stream.d_col, A->stream.d_val, (int32_t)A->rows, (int32_t)A->cols};
  const uint32_t *yp = use_y ? (const uint32_t *)Y->d : nullptr;
  const int grid = A->stream.n_stream + A->stream.n_segs;
  if (grid > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_csr_kernel<SR, K>), dim3(grid), dim3(BS), 0, e->stream, dev, (const uint32_t *)X->d, yp,
                       alpha, beta, use_y ? 1 : 0, (uint32_t *)Out->d, A->stream.d_blk_row, A->stream.n_stream, A->stream.d_segs, A->stream.d_partial_multi, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (A->stream.n_long > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(spmm_long_fixup<SR, K>), dim3((A->stream.n_long * K + 63) / 64), dim3(64), 0, e->stream, A->stream.d_long,
                       A->stream.n_long, A->stream.d_partial_multi, yp, alpha, beta, use_y ? 1 : 0, (uint32_t *)Out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

template <class SR>
static int launch_spmm_width(sh_engine *e, const sh_csr *A, int32_t width, const sh_vec *X, const sh_vec *Y, const void *alpha,
                             const void *beta, sh_vec *Out, MultiStep st) {
  switch (width) {
  case 4: return launch_spmm<SR, 4>(e, A, X, Y, alpha, beta, Out, st);
  case 8: return launch_spmm<SR, 8>(e, A, X, Y, alpha, beta, Out, st);
  case 16: return launch_spmm<SR, 16>(e, A, X, Y, alpha, beta, Out, st);
  case 32: return launch_spmm<SR, 32>(e, A, X, Y, alpha, beta, Out, st);
  default: return fail(e, SH_EINVAL, "width %d: sh_spmm serves 4, 8, 16 or 32 vectors per launch", (int)width);
  }
}

static int dispatch_spmm(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, const sh_vec *X, const sh_vec *Y,
                         const void *alpha, const void *beta, sh_vec *Out, MultiStep st) {
  switch (sr) {
  case SH_PLUS_TIMES_F32: return launch_spmm_width<PlusTimesF32>(e, A, width, X, Y, alpha, beta, Out, st);
  case SH_MIN_PLUS_F32: return launch_spmm_width<MinPlusF32>(e, A, width, X, Y, alpha, beta, Out, st);
  case SH_OR_AND_I32: return launch_spmm_width<OrAndI32>(e, A, width, X, Y, alpha, beta, Out, st);
  case SH_MAX_MIN_I32: return launch_spmm_width<MaxMinI32>(e, A, width, X, Y, alpha, beta, Out, st);
  default: return fail(e, SH_EINVAL, "unknown semiring %d", (int)sr);
  }
}

// What sh_spmm and sh_iterate_multi ask of their operands (Y == NULL is legal where the epilogue does not read it).
static int check_multi(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, const sh_vec *X, const sh_vec *Y,
                       const void *alpha, const void *beta, const sh_vec *Out, const char *who) {
  if (!e || !A || !X || !alpha || !beta || !Out)
    return fail(e, SH_EINVAL, "%s: NULL argument", who);
  if ((int)sr < SH_PLUS_TIMES_F32 || (int)sr > SH_MAX_MIN_I32)
    return fail(e, SH_EINVAL, "%s: unknown semiring %d", who, (int)sr);
  if (width != 4 && width != 8 && width != 16 && width != 32)
    return fail(e, SH_EINVAL, "%s: width %d, must be 4, 8, 16 or 32", who, (int)width);
  if (!A->stream.d_row_ptr || !A->stream.d_blk_row)
    return fail(e, SH_EINVAL, "%s: the matrix does not hold its CSR arrays on the device (it runs the tiled or the bit-blocked "
                "plan); upload it with sh_plan_options::plan = 1 (SH_PLAN=stream)", who);
  const bool use_y = reads_y(sr, beta);
  if (use_y && !Y)
    return fail(e, SH_EINVAL, "%s: Y is NULL but the epilogue reads it (beta != 0 or min-plus)", who);
  if (X->n < A->cols * width)
    return fail(e, SH_ESHAPE, "%s: X has %lld elements, needs cols * width = %lld", who, (long long)X->n, (long long)(A->cols * width));
  if (Out->n < A->rows * width)
    return fail(e, SH_ESHAPE, "%s: Out has %lld elements, needs rows * width = %lld", who, (long long)Out->n, (long long)(A->rows * width));
  if (use_y && Y->n < A->rows * width)
    return fail(e, SH_ESHAPE, "%s: Y has %lld elements, needs rows * width = %lld", who, (long long)Y->n, (long long)(A->rows * width));
  if (Out->d == X->d && A->rows > 0)
    return fail(e, SH_EINVAL, "%s: Out must not alias X", who);
  for (const sh_vec *v : {X, use_y ? Y : X, Out})
    if ((uintptr_t)v->d % 16 != 0)
      return fail(e, SH_EINVAL, "%s: vectors must be 16-byte aligned (a lane moves four columns at a time)", who);
  return SH_OK;
}

extern "C" {

int sh_spmm(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, const sh_vec *X, const sh_vec *Y,
            const void *alpha, const void *beta, sh_vec *Out, uint64_t *kernel_ns) {
  int rc = check_multi(e, sr, A, width, X, Y, alpha, beta, Out, "sh_spmm");
  if (rc)
    return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  if (kernel_ns)
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  rc = dispatch_spmm(e, sr, A, width, X, Y, alpha, beta, Out, MultiStep{nullptr, nullptr, 0.0, nullptr});
  if (rc)
    return rc;
  if (kernel_ns) {
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ns = (uint64_t)((double)ms * 1e6);
  }
  return SH_OK;
}

int sh_iterate_multi(sh_engine *e, sh_semiring sr, const sh_csr *A, int32_t width, sh_vec *X, const sh_vec *Y0,
                     sh_vec *scratch, const void *alpha, const void *beta, double delta, int32_t max_iters,
                     int32_t *launches, int32_t *iters_of_column, int32_t *converged_of_column,
                     uint64_t *ns_per_launch, uint64_t *total_ns) {
  if (!Y0 || !scratch || !launches || !iters_of_column || !converged_of_column)
    return fail(e, SH_EINVAL, "sh_iterate_multi: NULL argument");
  int rc = check_multi(e, sr, A, width, X, Y0, alpha, beta, scratch, "sh_iterate_multi");
  if (rc)
    return rc;
  if (A->rows != A->cols)
    return fail(e, SH_ESHAPE, "sh_iterate_multi: matrix must be square (inc/common.h:49-52)");
  if (Y0->n < A->rows * width)
    return fail(e, SH_ESHAPE, "sh_iterate_multi: Y0 has %lld elements, needs rows * width = %lld", (long long)Y0->n, (long long)(A->rows * width));
  if ((uintptr_t)Y0->d % 16 != 0)
    return fail(e, SH_EINVAL, "sh_iterate_multi: vectors must be 16-byte aligned (a lane moves four columns at a time)");
  *launches = 0;
  for (int j = 0; j < width; j++) iters_of_column[j] = 0, converged_of_column[j] = 0;
  if (total_ns)
    *total_ns = 0;
  if (max_iters <= 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  constexpr int SLOT = SPMM_MAX_WIDTH, MULTI_FLAG_WORDS = (8 + 1) * SLOT;   // (iterate_slots: 8 launches to a batch)
  HIP_TRY(e, e->dense.mflags.open(MULTI_FLAG_WORDS * 4));
  PingPong pp{X, scratch, Y0};
  DenseRun run;
  auto launch = [&](int, const PingPong &p, int32_t *flags, const int32_t *active) -> int {
    return dispatch_spmm(e, sr, A, width, p.in, p.y, alpha, beta, p.out, MultiStep{flags, (const uint32_t *)p.in->d, delta, active});
  };
  auto flag = [](const int32_t *slot, int j) { return slot[j] != 0; };
  RC_TRY(iterate_slots<SLOT>(e, pp, e->dense.mflags, MULTI_FLAG_WORDS, MULTI_FLAG_WORDS, width, max_iters, iters_of_column,
                             converged_of_column, ns_per_launch, &run, launch, flag, [](int32_t, int) {}));
  RC_TRY(pp.hand_back(e, X, (size_t)A->rows * width * 4));
  *launches = run.launches;
  if (total_ns)
    *total_ns = run.total_ns;
  return SH_OK;
}

} // extern "C"

// ---- (or,and) on packed bits (msbfs.hip.h) -------------------------------------------------------------------------
constexpr int BITS_MAX_WORDS = 8;   // widest sh_bits_spmv: 256 sources
static_assert(BITS_MAX_WORDS <= SPMM_MAX_WIDTH, "the long-row partials live in d_partial_multi");

template <int W, bool COUNTS>
static int launch_bits(sh_engine *e, const sh_csr *A, const sh_vec *X, const sh_vec *Y, uint32_t amask, uint32_t bmask,
                       sh_vec *Out, BitsStep st) {
  CsrDev dev{A->stream.d_row_ptr, A->stream.d_col, A->stream.d_val, (int32_t)A->rows, (int32_t)A->cols};
  const uint32_t *yp = bmask ? (const uint32_t *)Y->d : nullptr;
  const int grid = A->stream.n_stream + A->stream.n_segs;
  if (grid > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(msbfs_csr_kernel<W, COUNTS>), dim3(grid), dim3(BS), 0, e->stream, dev, (const uint32_t *)X->d, yp,
                       amask, bmask, (uint32_t *)Out->d, A->stream.d_blk_row, A->stream.n_stream, A->stream.d_segs, A->stream.d_partial_multi, st);
    HIP_TRY(e, hipGetLastError());
  }
  if (A->stream.n_long > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(msbfs_long_fixup<W, COUNTS>), dim3((A->stream.n_long * W + 63) / 64), dim3(64), 0, e->stream, A->stream.d_long,
                       A->stream.n_long, A->stream.d_partial_multi, yp, amask, bmask, (uint32_t *)Out->d, st);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

template <bool COUNTS>
static int launch_bits_words(sh_engine *e, const sh_csr *A, int32_t words, const sh_vec *X, const sh_vec *Y, uint32_t amask,
                             uint32_t bmask, sh_vec *Out, BitsStep st) {
  switch (words) {
  case 1: return launch_bits<1, COUNTS>(e, A, X, Y, amask, bmask, Out, st);
  case 2: return launch_bits<2, COUNTS>(e, A, X, Y, amask, bmask, Out, st);
  case 4: return launch_bits<4, COUNTS>(e, A, X, Y, amask, bmask, Out, st);
  case 8: return launch_bits<8, COUNTS>(e, A, X, Y, amask, bmask, Out, st);
  default: return fail(e, SH_EINVAL, "words %d: 1, 2, 4 or 8 words per vertex", (int)words);
  }
}

static bool bits_words_ok(int32_t words) { return words == 1 || words == 2 || words == 4 || words == 8; }

// What sh_bits_spmv and sh_bits_iterate ask of their operands (Y == NULL is legal when beta == 0).
static int check_bits(sh_engine *e, const sh_csr *A, int32_t words, const sh_vec *X, const sh_vec *Y, const void *alpha,
                      const void *beta, const sh_vec *Out, const char *who) {
  if (!bits_words_ok(words))   // (by value first: refused without an engine too)
    return fail(e, SH_EINVAL, "%s: words %d, must be 1, 2, 4 or 8", who, (int)words);
  if (!e || !A || !X || !alpha || !beta || !Out)
    return fail(e, SH_EINVAL, "%s: NULL argument", who);
  if (!A->stream.d_row_ptr || !A->stream.d_blk_row)
    return fail(e, SH_EINVAL, "%s: the matrix does not hold its CSR arrays on the device (it runs the tiled or the bit-blocked "
                "plan); upload it with sh_plan_options::plan = 1 (SH_PLAN=stream)", who);
  int32_t b;
  memcpy(&b, beta, 4);
  const bool use_y = OrAndI32::reads_y(b);
  if (use_y && !Y)
    return fail(e, SH_EINVAL, "%s: Y is NULL but the epilogue reads it (beta != 0)", who);
  if (X->n < A->cols * words)
    return fail(e, SH_ESHAPE, "%s: X has %lld elements, needs cols * words = %lld", who, (long long)X->n, (long long)(A->cols * words));
  if (Out->n < A->rows * words)
    return fail(e, SH_ESHAPE, "%s: Out has %lld elements, needs rows * words = %lld", who, (long long)Out->n, (long long)(A->rows * words));
  if (use_y && Y->n < A->rows * words)
    return fail(e, SH_ESHAPE, "%s: Y has %lld elements, needs rows * words = %lld", who, (long long)Y->n, (long long)(A->rows * words));
  if (Out->d == X->d && A->rows > 0)
    return fail(e, SH_EINVAL, "%s: Out must not alias X", who);
  for (const sh_vec *v : {X, use_y ? Y : X, Out})
    if ((uintptr_t)v->d % 16 != 0)
      return fail(e, SH_EINVAL, "%s: vectors must be 16-byte aligned (a lane moves up to four words at a time)", who);
  return SH_OK;
}

static void bits_masks(const void *alpha, const void *beta, uint32_t *amask, uint32_t *bmask) {
  int32_t a, b;
  memcpy(&a, alpha, 4);
  memcpy(&b, beta, 4);
  *amask = a != 0 ? ~0u : 0u;
  *bmask = b != 0 ? ~0u : 0u;
}

extern "C" {

int sh_bits_spmv(sh_engine *e, const sh_csr *A, int32_t words, const sh_vec *X, const sh_vec *Y, const void *alpha,
                 const void *beta, sh_vec *Out, uint64_t *kernel_ns) {
  int rc = check_bits(e, A, words, X, Y, alpha, beta, Out, "sh_bits_spmv");
  if (rc)
    return rc;
  uint32_t amask, bmask;
  bits_masks(alpha, beta, &amask, &bmask);
  HIP_TRY(e, hipSetDevice(e->device));
  if (kernel_ns)
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  rc = launch_bits_words<false>(e, A, words, X, Y, amask, bmask, Out, BitsStep{nullptr, nullptr, nullptr, nullptr});
  if (rc)
    return rc;
  if (kernel_ns) {
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ns = (uint64_t)((double)ms * 1e6);
  }
  return SH_OK;
}

int sh_bits_iterate(sh_engine *e, const sh_csr *A, int32_t words, sh_vec *X, const sh_vec *Y0, sh_vec *scratch,
                    const void *alpha, const void *beta, int32_t max_iters, int32_t *launches,
                    int32_t *iters_of_source, int32_t *converged_of_source, uint32_t *newly_set,
                    uint64_t *ns_per_launch, uint64_t *total_ns) {
  if (!bits_words_ok(words))
    return fail(e, SH_EINVAL, "sh_bits_iterate: words %d, must be 1, 2, 4 or 8", (int)words);
  if (!Y0 || !scratch || !launches || !iters_of_source || !converged_of_source)
    return fail(e, SH_EINVAL, "sh_bits_iterate: NULL argument");
  int rc = check_bits(e, A, words, X, Y0, alpha, beta, scratch, "sh_bits_iterate");
  if (rc)
    return rc;
  if (A->rows != A->cols)
    return fail(e, SH_ESHAPE, "sh_bits_iterate: matrix must be square (inc/common.h:49-52)");
  if (Y0->n < A->rows * words)
    return fail(e, SH_ESHAPE, "sh_bits_iterate: Y0 has %lld elements, needs rows * words = %lld", (long long)Y0->n, (long long)(A->rows * words));
  if ((uintptr_t)Y0->d % 16 != 0)
    return fail(e, SH_EINVAL, "sh_bits_iterate: vectors must be 16-byte aligned (a lane moves up to four words at a time)");
  const int n_src = 32 * words;
  *launches = 0;
  for (int s = 0; s < n_src; s++) iters_of_source[s] = 0, converged_of_source[s] = 0;
  if (total_ns)
    *total_ns = 0;
  if (max_iters <= 0)
    return SH_OK;
  if (newly_set)
    memset(newly_set, 0, (size_t)max_iters * n_src * 4);
  uint32_t amask, bmask;
  bits_masks(alpha, beta, &amask, &bmask);
  HIP_TRY(e, hipSetDevice(e->device));
  // Behind the slots of iterate_slots (8 launches to a batch): 32 * BITS_MAX_WORDS level counts per launch of the batch.
  constexpr int SLOT = BITS_MAX_WORDS, CNT = 32 * BITS_MAX_WORDS, CNT0 = (8 + 1) * SLOT, BITS_STATE_WORDS = CNT0 + 8 * CNT;
  HIP_TRY(e, e->dense.bstate.open(BITS_STATE_WORDS * 4));
  const BatchWords<uint32_t> &bs = e->dense.bstate;
  PingPong pp{X, scratch, Y0};
  DenseRun run;
  auto launch = [&](int k, const PingPong &p, uint32_t *changed, const uint32_t *live) -> int {
    BitsStep st{changed, (const uint32_t *)p.in->d, live, bs.d + CNT0 + k * CNT};
    return newly_set ? launch_bits_words<true>(e, A, words, p.in, p.y, amask, bmask, p.out, st)
                     : launch_bits_words<false>(e, A, words, p.in, p.y, amask, bmask, p.out, st);
  };
  auto flag = [](const uint32_t *slot, int s) { return ((slot[s >> 5] >> (s & 31)) & 1u) != 0u; };
  auto counts = [&](int32_t l, int k) {
    if (newly_set)   // (the kernel's counts are word-major, 32 per word: source s at s)
      memcpy(newly_set + (size_t)l * n_src, bs.h + CNT0 + k * CNT, (size_t)n_src * 4);
  };
  RC_TRY(iterate_slots<SLOT>(e, pp, bs, BITS_STATE_WORDS, newly_set ? BITS_STATE_WORDS : CNT0, n_src, max_iters, iters_of_source,
                             converged_of_source, ns_per_launch, &run, launch, flag, counts));
  if (A->rows > 0)
    RC_TRY(pp.hand_back(e, X, (size_t)A->rows * words * 4));
  *launches = run.launches;
  if (total_ns)
    *total_ns = run.total_ns;
  return SH_OK;
}

static int check_bits_column(sh_engine *e, const sh_vec *packed, const sh_vec *column, int64_t n, int32_t words, int32_t source,
                             const char *who) {
  if (!bits_words_ok(words))   // (by value first: refused without an engine too)
    return fail(e, SH_EINVAL, "%s: words %d, must be 1, 2, 4 or 8", who, (int)words);
  if (source < 0 || source >= 32 * words)
    return fail(e, SH_EINVAL, "%s: source %d outside [0, 32 * words = %d)", who, (int)source, 32 * (int)words);
  if (!e || !packed || !column)
    return fail(e, SH_EINVAL, "%s: NULL argument", who);
  if (n < 0)
    return fail(e, SH_EINVAL, "%s: n is negative", who);
  if (column->n < n || packed->n < n * words)
    return fail(e, SH_ESHAPE, "%s: the column needs n = %lld elements, the packed vector n * words = %lld", who, (long long)n,
                (long long)(n * words));
  return SH_OK;
}

int sh_bits_from_column(sh_engine *e, const sh_vec *v, int64_t n, int32_t words, int32_t source, sh_vec *B) {
  const int rc = check_bits_column(e, B, v, n, words, source, "sh_bits_from_column");
  if (rc || n == 0)
    return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(msbfs_pack_column, dim3((unsigned)((n + BS - 1) / BS)), dim3(BS), 0, e->stream, (const uint32_t *)v->d, n, words,
                     source, (uint32_t *)B->d);
  HIP_TRY(e, hipGetLastError());
  return SH_OK;
}

int sh_bits_to_column(sh_engine *e, const sh_vec *B, int64_t n, int32_t words, int32_t source, sh_vec *v) {
  const int rc = check_bits_column(e, B, v, n, words, source, "sh_bits_to_column");
  if (rc || n == 0)
    return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  hipLaunchKernelGGL(msbfs_unpack_column, dim3((unsigned)((n + BS - 1) / BS)), dim3(BS), 0, e->stream, (const uint32_t *)B->d, n, words,
                     source, (uint32_t *)v->d);
  HIP_TRY(e, hipGetLastError());
  return SH_OK;
}

} // extern "C"

#ifdef SH_PLAN_EMULATE
#include "debug_tools.h"
#endif


// ---- what the worklist handles share (worklist.hip.h) ----------------------------------------------------------------
// What every sh_*_footprint / _edges / _max_forward / _max_degree / _delta accessor is: SH_EINVAL for a NULL handle or
// out pointer (no message is set: there is no engine to hold one), else the value.
#define HANDLE_GET(h, out, value) ((h) && (out) ? (*(out) = (value), (int)SH_OK) : (int)SH_EINVAL)

// The transpose of the pattern ptr / col with `n` entries (and of its weights when w != NULL): column histogram,
// exclusive scan, scatter through per-column cursors.  Enqueued only: `tmp` lives until the stream has been synchronised.
static int build_transpose(sh_engine *e, DevArrays &tmp, const int32_t *ptr, const int32_t *col, const uint32_t *w, int64_t n,
                           int64_t rows, int64_t cols, int32_t *out_ptr, int32_t *out_row, uint32_t *out_w) {
  uint32_t *cnt = nullptr;   // column counts, then the scatter's cursors
  HIP_TRY(e, tmp.alloc(&cnt, (cols + 1) * 4));
  HIP_TRY(e, hipMemsetAsync(cnt, 0, (size_t)(cols + 1) * 4, e->stream));
  const dim3 grid((unsigned)std::max<int64_t>(1, (n + WL_BS - 1) / WL_BS)), blk(WL_BS);
  if (n > 0) {
    hipLaunchKernelGGL(wl_col_hist, grid, blk, 0, e->stream, col, n, (int32_t)cols, cnt);
    HIP_TRY(e, hipGetLastError());
  }
  HIP_TRY(e, device_exclusive_sum_u32(e->stream, cnt, (uint32_t *)out_ptr, cols + 1));
  HIP_TRY(e, hipMemcpyAsync(cnt, out_ptr, (size_t)(cols + 1) * 4, hipMemcpyDeviceToDevice, e->stream));
  if (n > 0) {
    hipLaunchKernelGGL(wl_transpose_scatter, grid, blk, 0, e->stream, ptr, col, w, n, (int32_t)rows, (int32_t)cols, cnt, out_row, out_w);
    HIP_TRY(e, hipGetLastError());
  }
  return SH_OK;
}

// What sh_bfs_graph, sh_sssp_graph, sh_scc_graph and sh_wcc_graph share: the edges by row (in_*) and by source vertex (out_*), the static pieces of
// the long rows, and what a batch of gated steps needs (run_batches).  sh_core_graph keeps its symmetric lists in in_* alone.
// What every sh_*_graph has: the shape it was made from, the edges it kept, and the device arrays it owns.
struct GraphBase {
  int64_t rows = 0, nnz = 0, edges = 0;
  DevArrays dev;   // (dev_arrays.h; released after whatever a derived handle's destructor lets go of)
};

template <class Ctl>
struct GraphHandle : GraphBase {
  int32_t *d_in_ptr = nullptr, *d_in_col = nullptr, *d_out_ptr = nullptr, *d_out_row = nullptr;
  uint32_t *d_in_w = nullptr, *d_out_w = nullptr;   // |a| of every edge (NULL in a handle without weights)
  WlPiece *d_rpieces = nullptr;                     // pieces of the rows above the handle's row piece size (static)
  int32_t n_rpieces = 0;
  Ctl *d_ctl = nullptr;            // the control block, followed by the WlParts (and whatever else the handle puts there)
  WlPart *d_part = nullptr;
  Ctl *h_ctl = nullptr;            // pinned: the control block as read back once per batch
  hipEvent_t ev[sizeof(Ctl::rec) / sizeof(Ctl::rec[0]) + 1] = {};
  ~GraphHandle() {
    if (h_ctl) (void)hipHostFree(h_ctl);
    for (auto v : ev)
      if (v) (void)hipEventDestroy(v);
  }
};

// What the scalars and the host arrays of fn = sh_bfs_graph_create / ... / sh_core_graph_create / sh_truss_graph_create alone decide: no device is
// needed to be told.
static int check_host_csr(sh_engine *e, const char *fn, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, const void *out) {
  if (rows < 0 || rows > 0x7FFFFF00ll)
    return fail(e, SH_EINVAL, "%s: rows = %lld, must be in [0, 2^31 - 256]", fn, (long long)rows);
  if (nnz < 0 || nnz > 0x7FFFFF00ll)
    return fail(e, SH_EINVAL, "%s: nnz = %lld, must be in [0, 2^31 - 256]", fn, (long long)nnz);
  if (!row_ptr || !out || (nnz > 0 && (!col_idx || !val)))
    return fail(e, SH_EINVAL, "%s: NULL argument (row_ptr, out, or col_idx / val of a matrix with entries)", fn);
  if (row_ptr[0] != 0 || (int64_t)row_ptr[rows] != nnz)
    return fail(e, SH_ESHAPE, "%s: row_ptr[0] = %d and row_ptr[rows] = %d, must be 0 and nnz = %lld", fn, (int)row_ptr[0],
                (int)row_ptr[rows], (long long)nnz);
  for (int64_t r = 0; r < rows; r++)   // (the build indexes by row_ptr on the device: it must stay inside the arrays)
    if (row_ptr[r] > row_ptr[r + 1])
      return fail(e, SH_ESHAPE, "%s: row_ptr decreases at row %lld", fn, (long long)r);
  if (!e)
    return fail(e, SH_EINVAL, "%s: NULL argument (engine)", fn);
  return SH_OK;
}

// The edge lists of a graph handle from host CSR arrays: the entries that are edges (KEEP, see wl_edge_flag) by flag,
// exclusive scan and compaction (the stored order of the survivors is kept), the static pieces of long rows, the
// transpose; all with the weights |a| when `weights`.  ROW_PIECE: the handle's piece size for rows.  Returns with the
// stream synchronised: the host arrays are done with.
template <class KEEP, int ROW_PIECE, class Ctl>
static int build_edge_lists(sh_engine *e, GraphHandle<Ctl> *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                            const void *val, bool weights) {
  g->rows = rows; g->nnz = nnz;
  // temporaries: the CSR arrays as given, the edge flags and their scan, the cursor of the row pieces
  DevArrays tmp;
  int32_t *t_rp = nullptr, *t_ci = nullptr;
  uint32_t *t_val = nullptr, *t_flag = nullptr, *t_pos = nullptr, *t_cur = nullptr;
  HIP_TRY(e, tmp.alloc(&t_rp, (rows + 1) * 4));
  HIP_TRY(e, tmp.alloc(&t_ci, nnz * 4));
  HIP_TRY(e, tmp.alloc(&t_val, nnz * 4));
  HIP_TRY(e, tmp.alloc(&t_flag, (nnz + 1) * 4));
  HIP_TRY(e, tmp.alloc(&t_pos, (nnz + 1) * 4));
  HIP_TRY(e, tmp.alloc(&t_cur, 4));
  HIP_TRY(e, hipMemcpyAsync(t_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
  if (nnz > 0) {
    HIP_TRY(e, hipMemcpyAsync(t_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
  }
  HIP_TRY(e, hipMemsetAsync(t_cur, 0, 4, e->stream));
  const dim3 blk(WL_BS), ngrid((unsigned)((nnz + 1 + WL_BS - 1) / WL_BS)), rgrid((unsigned)((rows + 1 + WL_BS - 1) / WL_BS));
  hipLaunchKernelGGL(HIP_KERNEL_NAME(wl_edge_flag<KEEP>), ngrid, blk, 0, e->stream, t_ci, t_val, nnz, (int32_t)rows, t_flag);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, nnz + 1));
  uint32_t n_edges = 0;
  HIP_TRY(e, hipMemcpy(&n_edges, t_pos + nnz, 4, hipMemcpyDeviceToHost));
  const int64_t E = (int64_t)n_edges;
  g->edges = E;
  DevArrays &own = g->dev;
  HIP_TRY(e, own.alloc(&g->d_in_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_in_col, E * 4));
  if (weights) HIP_TRY(e, own.alloc(&g->d_in_w, E * 4));
  HIP_TRY(e, own.alloc(&g->d_out_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_out_row, E * 4));
  if (weights) HIP_TRY(e, own.alloc(&g->d_out_w, E * 4));
  HIP_TRY(e, own.alloc(&g->d_rpieces, (E / (ROW_PIECE / 2) + 1) * sizeof(WlPiece)));   // see wl_push_pieces
  if (nnz > 0) {
    hipLaunchKernelGGL(wl_edge_compact, ngrid, blk, 0, e->stream, t_ci, t_val, t_flag, t_pos, nnz, g->d_in_col, g->d_in_w);
    HIP_TRY(e, hipGetLastError());
  }
  hipLaunchKernelGGL(wl_row_starts, rgrid, blk, 0, e->stream, t_rp, t_pos, rows, g->d_in_ptr);
  HIP_TRY(e, hipGetLastError());
  if (rows > 0) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wl_row_pieces<ROW_PIECE>), rgrid, blk, 0, e->stream, g->d_in_ptr, rows, t_cur, g->d_rpieces);
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t n_rp = 0;
  HIP_TRY(e, hipMemcpyAsync(&n_rp, t_cur, 4, hipMemcpyDeviceToHost, e->stream));
  const int rc = build_transpose(e, tmp, g->d_in_ptr, g->d_in_col, g->d_in_w, E, rows, rows, g->d_out_ptr, g->d_out_row, g->d_out_w);
  if (rc)
    return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->n_rpieces = (int32_t)n_rp;
  return SH_OK;
}

// The control block of a graph handle (`nbytes` of device memory, zeroed), its pinned copy and the events of a batch.
template <class Ctl>
static int open_control(sh_engine *e, GraphHandle<Ctl> *g, int64_t ctl_bytes, int64_t nbytes) {
  HIP_TRY(e, g->dev.alloc(&g->d_ctl, nbytes));
  g->d_part = (WlPart *)((char *)g->d_ctl + ctl_bytes);
  HIP_TRY(e, hipHostMalloc((void **)&g->h_ctl, sizeof(Ctl), hipHostMallocDefault));
  for (auto &ev : g->ev) HIP_TRY(e, hipEventCreate(&ev));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, (size_t)nbytes, e->stream));
  return SH_OK;
}

// What fn = sh_bfs_graph_create / ... / sh_truss_graph_create share: *out is cleared, the host arrays are checked
// (check_host_csr), the handle is made, build(g) fills it, and once the stream has drained the handle is the caller's.
// On any error the handle and what it allocated so far are released and *out stays NULL.  (A build that has to wait for
// the stream itself, as sh_sssp_graph's for its weight sum and sh_tri_graph's for its longest list, leaves it idle.)
template <class H, class Build>
static int create_graph_handle(sh_engine *e, const char *fn, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                               const void *val, H **out, Build build) {
  if (out) *out = nullptr;
  int rc = check_host_csr(e, fn, rows, nnz, row_ptr, col_idx, val, out);
  if (rc)
    return rc;
  HIP_TRY(e, hipSetDevice(e->device));
  std::unique_ptr<H> g(new (std::nothrow) H());
  if (!g)
    return fail(e, SH_ENOMEM, "out of host memory");
  if ((rc = build(g.get())))
    return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  *out = g.release();
  return SH_OK;
}

// The loop of sh_bfs_levels, sh_sssp, sh_scc, sh_wcc, sh_core, sh_truss, sh_color, sh_msf, sh_match, sh_rcm, sh_bc and the analysis of sh_trsv_graph_create: batches of gated steps enqueued ahead of the host (the first batch holds 8, the
// next ones twice as many up to the records the control block has).  Per batch: the records are cleared, enqueue(s, k)
// enqueues step s as slot k, the control block is copied back, and take(s, rec, ns) gets the record and the time of every
// step that ran.  The launches between e->ev0 and e->ev1 (the caller's init) are timed from the first batch's readback.
// `what`: "<function>: <step>" for the error of a step that did not report.
template <class Ctl, class Enqueue, class Take>
static int run_batches(sh_engine *e, const char *what, GraphHandle<Ctl> *g, int32_t cap, int32_t *steps, bool *finished, uint64_t *total,
                       Enqueue enqueue, Take take) {
  constexpr int32_t MAX_BATCH = sizeof(Ctl::rec) / sizeof(Ctl::rec[0]);
  int32_t it = 0, batch = 8;
  bool done = false;
  uint64_t ns = 0;
  while (!done && it < cap) {
    const int nb = std::min<int32_t>(batch, cap - it);
    HIP_TRY(e, hipMemsetAsync((char *)g->d_ctl + offsetof(Ctl, rec), 0, sizeof(Ctl::rec), e->stream));
    HIP_TRY(e, hipEventRecord(g->ev[0], e->stream));
    for (int k = 0; k < nb; k++) {
      const int rc = enqueue(it + k, k);
      if (rc)
        return rc;
      HIP_TRY(e, hipEventRecord(g->ev[k + 1], e->stream));
    }
    HIP_TRY(e, hipMemcpyAsync(g->h_ctl, g->d_ctl, sizeof(Ctl), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (batch == 8) {   // (the first batch)
      HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
      *total += ns;
    }
    int ran = 0;
    while (ran < nb && g->h_ctl->rec[ran].ran) ran++;
    for (int k = 0; k < ran; k++) {
      HIP_TRY(e, ms_between(g->ev[k], g->ev[k + 1], &ns));
      *total += ns;
      take(it + k, g->h_ctl->rec[k], ns);
    }
    it += ran;
    done = g->h_ctl->finished != 0;
    if (!done && ran < nb)
      return fail(e, SH_EHIP, "%s %d of the search did not report", what, (int)it);
    batch = std::min(batch * 2, MAX_BATCH);
  }
  *steps = it;
  *finished = done;
  return SH_OK;
}


// ---- frontier-driven iteration (frontier.hip.h) --------------------------------------------------------------------
struct sh_frontier {
  int64_t rows = 0, nnz = 0;
  const sh_csr *A = nullptr;       // the matrix the handle was made for
  bool borrowed = false;           // d_row_ptr / d_col / d_val are A's
  int32_t *d_row_ptr = nullptr, *d_col = nullptr;
  uint32_t *d_val = nullptr;
  int32_t *d_col_ptr = nullptr, *d_row_of = nullptr;
  uint32_t *d_clist = nullptr, *d_alist = nullptr, *d_stamp = nullptr, *d_side = nullptr;
  WlPiece *d_cplist = nullptr, *d_rplist = nullptr;
  FrontierCtl *d_ctl = nullptr;
  FrontierRec *h_rec = nullptr;    // pinned: the records of a batch
  uint32_t gen = 0;                // number of the latest sparse launch enqueued (what its stamps hold)
  DevArrays dev;                   // the arrays that are the handle's own
  ~sh_frontier() {
    if (h_rec) (void)hipHostFree(h_rec);
  }
};

// sh_iterate_frontier's dense_share < 0: see DESIGN.md "Frontier-driven iteration" (the sweep of tools/frontier_bench.py)
static constexpr double FRONTIER_DENSE_SHARE = 0.02;
static_assert(sizeof(FrontierCtl) <= FR_CTL_BYTES, "the control block is accounted as FR_CTL_BYTES (sh_frontier_footprint)");

template <class SR>
static int launch_sparse(sh_engine *e, sh_frontier *f, const sh_csr *A, sh_vec *cur, const void *alpha_p, const void *beta_p,
                         double delta, int k, int p) {
  using T = typename SR::T;
  T alpha, beta;
  memcpy(&alpha, alpha_p, 4);
  memcpy(&beta, beta_p, 4);
  if (++f->gen == 0) {   // the launch numbers wrapped: no stamp may look current
    HIP_TRY(e, hipMemsetAsync(f->d_stamp, 0, (size_t)std::max<int64_t>(f->rows, 1) * 4, e->stream));
    f->gen = 1;
  }
  const dim3 grid((unsigned)(e->n_cus * 4)), block(WL_BS);
  const CsrDev dev{f->d_row_ptr, f->d_col, f->d_val, (int32_t)A->rows, (int32_t)A->cols};
  hipLaunchKernelGGL(frontier_mark, grid, block, 0, e->stream, f->d_ctl, k, p, f->gen, (int32_t)A->rows, f->d_col_ptr, f->d_row_of,
                     f->d_row_ptr, f->d_clist, f->d_cplist, f->d_stamp, f->d_alist, f->d_side, f->d_rplist, (uint32_t)SR::identity_bits);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(HIP_KERNEL_NAME(frontier_pull<SR>), grid, block, 0, e->stream, f->d_ctl, k, dev, (const uint32_t *)cur->d,
                     f->d_alist, f->d_side, f->d_rplist);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(HIP_KERNEL_NAME(frontier_apply<SR>), grid, block, 0, e->stream, f->d_ctl, k, p ^ 1, (uint32_t *)cur->d, f->d_alist,
                     f->d_side, f->d_col_ptr, f->d_clist, f->d_cplist, alpha, beta, SR::reads_y(beta) ? 1 : 0, delta);
  HIP_TRY(e, hipGetLastError());
  return SH_OK;
}

extern "C" {

int sh_frontier_create(sh_engine *e, const sh_csr *A, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                       const void *val, sh_frontier **out) {
  if (!e || !A || !row_ptr || !out || (nnz > 0 && (!col_idx || !val)))
    return fail(e, SH_EINVAL, "sh_frontier_create: NULL argument");
  *out = nullptr;
  if (A->rows != A->cols)
    return fail(e, SH_ESHAPE, "sh_frontier_create: matrix must be square");
  if (nnz != A->nnz || row_ptr[0] != 0 || row_ptr[A->rows] != nnz)
    return fail(e, SH_ESHAPE, "sh_frontier_create: the arrays hold %lld entries, the matrix %lld", (long long)nnz, (long long)A->nnz);
  HIP_TRY(e, hipSetDevice(e->device));
  std::unique_ptr<sh_frontier> f(new (std::nothrow) sh_frontier());
  if (!f)
    return fail(e, SH_ENOMEM, "out of host memory");
  const int64_t rows = A->rows, cols = A->cols;
  f->rows = rows; f->nnz = nnz; f->A = A;
  DevArrays &own = f->dev, tmp;
  f->borrowed = A->stream.d_row_ptr && (nnz == 0 || (A->stream.d_col && A->stream.d_val));
  if (f->borrowed) {
    f->d_row_ptr = A->stream.d_row_ptr; f->d_col = A->stream.d_col; f->d_val = A->stream.d_val;
  } else {
    HIP_TRY(e, own.alloc(&f->d_row_ptr, (rows + 1) * 4));
    HIP_TRY(e, own.alloc(&f->d_col, nnz * 4));
    HIP_TRY(e, own.alloc(&f->d_val, nnz * 4));
    HIP_TRY(e, hipMemcpyAsync(f->d_row_ptr, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
    if (nnz > 0) {
      HIP_TRY(e, hipMemcpyAsync(f->d_col, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
      HIP_TRY(e, hipMemcpyAsync(f->d_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    }
  }
  HIP_TRY(e, own.alloc(&f->d_col_ptr, (cols + 1) * 4));
  HIP_TRY(e, own.alloc(&f->d_row_of, nnz * 4));
  HIP_TRY(e, own.alloc(&f->d_clist, rows * 4));
  HIP_TRY(e, own.alloc(&f->d_alist, rows * 4));
  HIP_TRY(e, own.alloc(&f->d_stamp, rows * 4));
  HIP_TRY(e, own.alloc(&f->d_side, rows * 4));
  HIP_TRY(e, own.alloc(&f->d_cplist, (nnz / 1024 + 1) * sizeof(WlPiece)));   // see wl_push_pieces: columns longer than 2048
  HIP_TRY(e, own.alloc(&f->d_rplist, (nnz / 2048 + 1) * sizeof(WlPiece)));   // the same for rows longer than 4096
  HIP_TRY(e, own.alloc(&f->d_ctl, FR_CTL_BYTES));
  HIP_TRY(e, hipHostMalloc((void **)&f->h_rec, sizeof(FrontierRec) * FR_BATCH, hipHostMallocDefault));
  HIP_TRY(e, hipMemsetAsync(f->d_stamp, 0, std::max<size_t>((size_t)rows * 4, 16), e->stream));
  HIP_TRY(e, hipMemsetAsync(f->d_ctl, 0, FR_CTL_BYTES, e->stream));
  const int rc = build_transpose(e, tmp, f->d_row_ptr, f->d_col, nullptr, nnz, rows, cols, f->d_col_ptr, f->d_row_of, nullptr);
  if (rc)
    return rc;
  HIP_TRY(e, hipStreamSynchronize(e->stream));   // the host arrays and the cursors are done with
  *out = f.release();
  return SH_OK;
}

int sh_frontier_free(sh_engine *e, sh_frontier *f) { return free_handle(e, f); }

int sh_frontier_footprint(const sh_frontier *f, uint64_t *device_bytes) { return HANDLE_GET(f, device_bytes, (uint64_t)f->dev.bytes); }

int sh_frontier_transpose(sh_engine *e, const sh_frontier *f, int32_t *col_ptr, int32_t *row_of) {
  if (!e || !f)
    return fail(e, SH_EINVAL, "sh_frontier_transpose: NULL argument");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  int32_t n = 0;
  HIP_TRY(e, hipMemcpy(&n, f->d_col_ptr + f->rows, 4, hipMemcpyDeviceToHost));
  if (col_ptr) HIP_TRY(e, hipMemcpy(col_ptr, f->d_col_ptr, (size_t)(f->rows + 1) * 4, hipMemcpyDeviceToHost));
  if (row_of && n > 0) HIP_TRY(e, hipMemcpy(row_of, f->d_row_of, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SH_OK;
}

int sh_iterate_frontier(sh_engine *e, sh_semiring sr, const sh_csr *A, sh_frontier *f, sh_vec *x, const sh_vec *y0,
                        sh_vec *scratch, const void *alpha, const void *beta, double delta, int32_t max_iters,
                        double dense_share, int32_t *iters, int32_t *converged, int32_t *mode_per_iter,
                        int64_t *changed_per_iter, int64_t *active_per_iter, uint64_t *ns_per_iter, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (sr == SH_PLUS_TIMES_F32)
    return fail(e, SH_EINVAL, "sh_iterate_frontier: SH_PLUS_TIMES_F32 is not served (a recomputed row would have to reproduce "
                              "the summation order of the dense launches' plan): call sh_iterate");
  if (sr != SH_MIN_PLUS_F32 && sr != SH_OR_AND_I32 && sr != SH_MAX_MIN_I32)
    return fail(e, SH_EINVAL, "sh_iterate_frontier: unknown semiring %d", (int)sr);
  if (max_iters < 1)
    return fail(e, SH_EINVAL, "sh_iterate_frontier: max_iters = %d, must be at least 1", (int)max_iters);
  if (sr == SH_MIN_PLUS_F32 && !(delta > 0.0))
    return fail(e, SH_EINVAL, "sh_iterate_frontier: delta = %g, SH_MIN_PLUS_F32 needs delta > 0 (a row that is not recomputed "
                              "must pass |in - out| < delta)", delta);
  if (!e || !A || !f || !x || !y0 || !scratch || !alpha || !beta || !iters || !converged)
    return fail(e, SH_EINVAL, "sh_iterate_frontier: NULL argument");
  if (A->rows != A->cols)
    return fail(e, SH_ESHAPE, "sh_iterate_frontier: matrix must be square (inc/common.h:49-52)");
  if (f->rows != A->rows || f->nnz != A->nnz || (f->borrowed && f->A != A))
    return fail(e, SH_EINVAL, "sh_iterate_frontier: the frontier handle was made for another matrix");
  if (x->n < A->rows || scratch->n < A->rows || y0->n < A->rows)
    return fail(e, SH_ESHAPE, "sh_iterate_frontier: vectors shorter than the matrix");
  if (scratch->d == x->d && A->rows > 0)
    return fail(e, SH_EINVAL, "sh_iterate_frontier: scratch must not alias x");
  HIP_TRY(e, hipSetDevice(e->device));
  if (dense_share < 0) dense_share = FRONTIER_DENSE_SHARE;
  const bool never_sparse = dense_share == 0.0;
  const uint32_t max_entries = dense_share >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(dense_share * (double)A->nnz);
  HIP_TRY(e, hipMemsetAsync(f->d_ctl, 0, FR_CTL_BYTES, e->stream));
  const dim3 dgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>((A->rows + WL_BS - 1) / WL_BS, (int64_t)e->n_cus * 8)));
  // A batch holds launches of ONE mode: which buffer a launch reads must be known when it is enqueued, and that
  // depends on how many dense launches (which swap the buffers) ran before it.
  bool sparse = false;
  PingPong pp{x, scratch, y0};
  DenseRun run;
  auto begin = [&]() -> int {
    hipLaunchKernelGGL(frontier_begin, dim3(1), dim3(64), 0, e->stream, f->d_ctl);
    HIP_TRY(e, hipGetLastError());
    return SH_OK;
  };
  auto enqueue = [&](int32_t L, int k, const PingPong &b, bool *swaps) -> int {
    const int p = L & 1;
    *swaps = !sparse;
    if (sparse) {
      switch (sr) {
      case SH_MIN_PLUS_F32: RC_TRY(launch_sparse<MinPlusF32>(e, f, A, b.in, alpha, beta, delta, k, p)); break;
      case SH_OR_AND_I32: RC_TRY(launch_sparse<OrAndI32>(e, f, A, b.in, alpha, beta, delta, k, p)); break;
      default: RC_TRY(launch_sparse<MaxMinI32>(e, f, A, b.in, alpha, beta, delta, k, p)); break;
      }
    } else {
      StepDev st{f->d_ctl->flag + k, (const uint32_t *)b.in->d, 0, delta, f->d_ctl->go + k};
      RC_TRY(dispatch(e, sr, A, b.in, b.y, alpha, beta, b.out, st));
      hipLaunchKernelGGL(frontier_detect, dgrid, dim3(WL_BS), 0, e->stream, f->d_ctl, k, p ^ 1, (const uint32_t *)b.in->d,
                         (const uint32_t *)b.out->d, (int32_t)A->rows, f->d_col_ptr, f->d_clist, f->d_cplist);
      HIP_TRY(e, hipGetLastError());
    }
    hipLaunchKernelGGL(frontier_decide, dim3(1), dim3(64), 0, e->stream, f->d_ctl, k, p, sparse ? 0 : 1, (int32_t)A->rows, max_entries,
                       (!never_sparse && L + 1 >= 2) ? 1 : 0, sparse ? 1 : 0);
    HIP_TRY(e, hipGetLastError());
    return SH_OK;
  };
  auto settle = [&](int32_t first, int nb, int *ran, bool *over) -> int {
    while (*ran < nb && f->h_rec[*ran].ran) ++*ran;
    if (*ran < 1)
      return fail(e, SH_EHIP, "sh_iterate_frontier: the first launch of a batch did not report");
    for (int k = 0; k < *ran; k++) {
      if (mode_per_iter) mode_per_iter[first + k] = sparse ? 1 : 0;
      if (changed_per_iter) changed_per_iter[first + k] = (int64_t)f->h_rec[k].changed;
      if (active_per_iter) active_per_iter[first + k] = (int64_t)f->h_rec[k].active;
    }
    *over = f->h_rec[*ran - 1].differs == 0;
    sparse = f->h_rec[*ran - 1].sparse_next != 0;
    return SH_OK;
  };
  RC_TRY(run_dense_batches<FR_BATCH>(e, pp, max_iters, Readback{f->h_rec, f->d_ctl->rec, sizeof(FrontierRec) * FR_BATCH}, ns_per_iter,
                                     &run, begin, enqueue, settle));
  RC_TRY(pp.hand_back(e, x, A->rows * 4));
  *iters = run.launches;
  *converged = run.over ? 1 : 0;
  if (total_ns)
    *total_ns = run.total_ns;
  return SH_OK;
}

} // extern "C"

// ---- direction-optimising BFS with levels and parents (bfs.hip.h) -----------------------------------------------------
struct sh_bfs_graph : GraphHandle<BfsCtl> {   // d_ctl: BFS_CTL_BYTES, followed by the WlParts
  int32_t words = 0;               // 32-bit words of one frontier bitmap
  uint32_t *d_queue[2] = {nullptr, nullptr}, *d_bm[2] = {nullptr, nullptr};
  WlPiece *d_opieces[2] = {nullptr, nullptr};   // pieces of the long out-lists of the frontier in queue 0 / 1
};
// sh_bfs_levels' up_share / down_share < 0: see DESIGN.md "6e Direction-optimising BFS" (the sweep of tools/bfs_levels_bench.py)
static constexpr double BFS_UP_SHARE = 0.005, BFS_DOWN_SHARE = 0.01;
static_assert(sizeof(BfsCtl) <= BFS_CTL_BYTES, "the control block is accounted as BFS_CTL_BYTES (sh_bfs_graph_footprint)");
static_assert(sizeof(WlPart) * BFS_MAX_BLOCKS == BFS_PART_BYTES, "one WlPart per workgroup");

extern "C" {

int sh_bfs_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_bfs_graph **out) {
  return create_graph_handle<sh_bfs_graph>(e, "sh_bfs_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_bfs_graph *g) -> int {
    int rc;
    g->words = (int32_t)((rows + 31) / 32);
    if ((rc = build_edge_lists<BfsKeep, BFS_ROW_PIECE>(e, g, rows, nnz, row_ptr, col_idx, val, false)))
      return rc;
    for (int i = 0; i < 2; i++) {
      HIP_TRY(e, g->dev.alloc(&g->d_queue[i], rows * 4));
      HIP_TRY(e, g->dev.alloc(&g->d_bm[i], (int64_t)g->words * 4));
      HIP_TRY(e, g->dev.alloc(&g->d_opieces[i], (g->edges / 1024 + 1) * sizeof(WlPiece)));   // see wl_push_pieces: out-lists longer than 2048
    }
    return open_control(e, g, BFS_CTL_BYTES, BFS_CTL_BYTES + BFS_PART_BYTES);
  });
}

int sh_bfs_graph_free(sh_engine *e, sh_bfs_graph *g) { return free_handle(e, g); }

int sh_bfs_graph_footprint(const sh_bfs_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_bfs_graph_edges(const sh_bfs_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_bfs_levels(sh_engine *e, sh_bfs_graph *g, const sh_vec *x0, sh_vec *level, sh_vec *parent, int32_t max_levels,
                  double up_share, double down_share, int32_t *depth, int64_t *reached, int32_t *complete,
                  int32_t *mode_per_level, int64_t *size_per_level, int64_t *edges_per_level, uint64_t *ns_per_level,
                  uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (max_levels < 1)
    return fail(e, SH_EINVAL, "sh_bfs_levels: max_levels = %d, must be at least 1", (int)max_levels);
  if (up_share != up_share || down_share != down_share)
    return fail(e, SH_EINVAL, "sh_bfs_levels: %s is NaN", up_share != up_share ? "up_share" : "down_share");
  if (!e || !g || !x0 || !level || !depth || !reached || !complete)
    return fail(e, SH_EINVAL, "sh_bfs_levels: NULL argument (engine, graph, x0, level, depth, reached or complete)");
  const int64_t rows = g->rows;
  if (x0->n < rows || level->n < rows || (parent && parent->n < rows))
    return fail(e, SH_ESHAPE, "sh_bfs_levels: %s is shorter than the graph's %lld rows",
                x0->n < rows ? "x0" : level->n < rows ? "level" : "parent", (long long)rows);
  if (rows > 0 && (level->d == x0->d || (parent && (parent->d == x0->d || parent->d == level->d))))
    return fail(e, SH_EINVAL, "sh_bfs_levels: level and parent must not alias x0 or each other");
  if (up_share < 0) up_share = BFS_UP_SHARE;
  if (down_share < 0) down_share = BFS_DOWN_SHARE;
  *depth = 0; *reached = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const double up_edges = up_share * (double)g->edges, down_rows = down_share * (double)rows;
  const int nblocks = std::max(1, std::min(e->n_cus * 4, BFS_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const dim3 dgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)g->words + WL_BS - 1) / WL_BS, 256)));
  uint64_t total = 0, ns = 0;
  // level from x0, the sources as queue 0 and bitmap 0, the direction of step 0
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, BFS_CTL_BYTES, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_bm[1], 0, (size_t)g->words * 4, e->stream));
  hipLaunchKernelGGL(bfs_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, g->words, (const uint32_t *)x0->d, (int32_t *)level->d,
                     g->d_out_ptr, g->d_queue[0], g->d_opieces[0], g->d_bm[0], g->d_part);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(bfs_decide, dim3(1), block, 0, e->stream, g->d_ctl, 0, -1, nblocks, g->d_part, g->d_bm[0], g->words, up_edges,
                     down_rows);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  int64_t n_found = 0;
  // the three launches of a step: each returns at once unless the control block says the step runs in its direction
  const auto enqueue = [&](int L, int k) {
    const int p = L & 1;
    hipLaunchKernelGGL(bfs_queue_from_bitmap, grid, block, 0, e->stream, g->d_ctl, L, g->words, g->d_bm[p], g->d_out_ptr, g->d_queue[p],
                       g->d_opieces[p]);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(bfs_topdown, grid, block, 0, e->stream, g->d_ctl, L, (int32_t *)level->d, g->d_out_ptr, g->d_out_row, g->d_queue[p],
                       g->d_opieces[p], g->d_queue[p ^ 1], g->d_opieces[p ^ 1], g->d_bm[p ^ 1], g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(bfs_bottomup, grid, block, 0, e->stream, g->d_ctl, L, (int32_t)rows, (int32_t *)level->d, g->d_in_ptr, g->d_in_col,
                       g->d_bm[p], g->d_bm[p ^ 1], g->d_rpieces, g->n_rpieces, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(bfs_decide, dgrid, block, 0, e->stream, g->d_ctl, k, L, nblocks, g->d_part, g->d_bm[p], g->words, up_edges,
                       down_rows);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int L, const BfsRec &rc, uint64_t step_ns) {
    if (ns_per_level) ns_per_level[L] = step_ns;
    if (mode_per_level) mode_per_level[L] = rc.mode;
    if (size_per_level) size_per_level[L + 1] = (int64_t)rc.found;
    if (edges_per_level) edges_per_level[L] = (int64_t)rc.edges;
    n_found += (int64_t)rc.found;
    if (rc.found > 0) *depth = L + 1;
  };
  const int rc = run_batches(e, "sh_bfs_levels: step", g, max_levels, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // (what bfs_init found: h_ctl is fresh because max_levels >= 1 makes run_batches read at least one batch back)
  if (size_per_level) size_per_level[0] = (int64_t)g->h_ctl->nsrc;
  if (parent) {
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    HIP_TRY(e, hipMemsetAsync(parent->d, 0xFF, (size_t)rows * 4, e->stream));
    hipLaunchKernelGGL(bfs_parents, grid, block, 0, e->stream, (int32_t)rows, (const int32_t *)level->d, g->d_in_ptr, g->d_in_col,
                       g->d_rpieces, g->n_rpieces, (int32_t *)parent->d);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
    total += ns;
  }
  *reached = (int64_t)g->h_ctl->nsrc + n_found;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- bucketed SSSP with distances and canonical predecessors (sssp.hip.h) --------------------------------------------
struct sh_sssp_graph : GraphHandle<SsspCtl> {   // d_ctl: SSSP_CTL_BYTES, followed by the WlParts and the split's minima
  double delta = 0.0;              // the default bucket width (0: no edges)
  uint32_t *d_stamp = nullptr, *d_near[2] = {nullptr, nullptr}, *d_far[2] = {nullptr, nullptr};
  WlPiece *d_opieces[2] = {nullptr, nullptr};   // pieces of the long out-lists of near list 0 / 1
  uint32_t *d_pmin = nullptr;
};
// The default bucket width is SSSP_DELTA_FACTOR * (mean weight) / (mean out-degree): Davidson et al.'s starting point.
// tools/sssp_bench.py sweeps the factor; no sweep is on record yet (DESIGN.md "6f Bucketed SSSP").
static constexpr double SSSP_DELTA_FACTOR = 32.0;
static_assert(sizeof(SsspCtl) <= SSSP_CTL_BYTES, "the control block is accounted as SSSP_CTL_BYTES (sh_sssp_graph_footprint)");
static_assert(sizeof(WlPart) * SSSP_MAX_BLOCKS == SSSP_PART_BYTES, "one WlPart per workgroup");

extern "C" {

int sh_sssp_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const void *val, sh_sssp_graph **out) {
  return create_graph_handle<sh_sssp_graph>(e, "sh_sssp_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_sssp_graph *g) -> int {
    int rc;
    if ((rc = build_edge_lists<SsspKeep, SSSP_ROW_PIECE>(e, g, rows, nnz, row_ptr, col_idx, val, true)))
      return rc;
    const int64_t E = g->edges;
    HIP_TRY(e, g->dev.alloc(&g->d_stamp, rows * 4));
    for (int i = 0; i < 2; i++) {
      HIP_TRY(e, g->dev.alloc(&g->d_near[i], rows * 4));
      HIP_TRY(e, g->dev.alloc(&g->d_far[i], rows * 4));
      HIP_TRY(e, g->dev.alloc(&g->d_opieces[i], (E / 1024 + 1) * sizeof(WlPiece)));   // see wl_push_pieces: out-lists longer than 2048
    }
    if ((rc = open_control(e, g, SSSP_CTL_BYTES, SSSP_CTL_BYTES + SSSP_PART_BYTES + SSSP_PMIN_BYTES)))
      return rc;
    g->d_pmin = (uint32_t *)((char *)g->d_ctl + SSSP_CTL_BYTES + SSSP_PART_BYTES);
    // the mean weight, for the default bucket width
    constexpr int SUM_BLOCKS = 256;
    DevArrays tmp;
    double *t_sum = nullptr, h_sum[SUM_BLOCKS] = {};
    HIP_TRY(e, tmp.alloc(&t_sum, SUM_BLOCKS * sizeof(double)));
    if (E > 0) {
      hipLaunchKernelGGL(sssp_weight_sum, dim3(SUM_BLOCKS), dim3(WL_BS), 0, e->stream, g->d_in_w, E, t_sum);
      HIP_TRY(e, hipGetLastError());
      HIP_TRY(e, hipMemcpyAsync(h_sum, t_sum, sizeof(h_sum), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // (h_sum and t_sum end with this scope: the sums must have landed)
    if (E > 0) {
      double sum = 0.0;
      for (double v : h_sum) sum += v;
      // factor * (sum / E) / (E / rows); a graph whose weights are all zero has one bucket whatever the width: 1
      const double d = SSSP_DELTA_FACTOR * (sum / (double)E) * ((double)rows / (double)E);
      g->delta = (d > 0.0 && d < 1e300) ? d : 1.0;
    }
    return SH_OK;
  });
}

int sh_sssp_graph_free(sh_engine *e, sh_sssp_graph *g) { return free_handle(e, g); }

int sh_sssp_graph_footprint(const sh_sssp_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_sssp_graph_edges(const sh_sssp_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_sssp_graph_delta(const sh_sssp_graph *g, double *delta) { return HANDLE_GET(g, delta, g->delta); }

int sh_sssp(sh_engine *e, sh_sssp_graph *g, const sh_vec *x0, sh_vec *dist, sh_vec *pred, double delta,
            int32_t max_rounds, int32_t *rounds, int32_t *buckets, int64_t *reached, int32_t *complete,
            int64_t *relaxed, int64_t *size_per_round, int64_t *edges_per_round, uint64_t *ns_per_round,
            uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_sssp: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (delta != delta)
    return fail(e, SH_EINVAL, "sh_sssp: delta is NaN");
  if (!e || !g || !x0 || !dist || !rounds || !buckets || !reached || !complete || !relaxed)
    return fail(e, SH_EINVAL, "sh_sssp: NULL argument (engine, graph, x0, dist, rounds, buckets, reached, complete or relaxed)");
  const int64_t rows = g->rows;
  if (x0->n < rows || dist->n < rows || (pred && pred->n < rows))
    return fail(e, SH_ESHAPE, "sh_sssp: %s is shorter than the graph's %lld rows",
                x0->n < rows ? "x0" : dist->n < rows ? "dist" : "pred", (long long)rows);
  if (rows > 0 && (dist->d == x0->d || (pred && (pred->d == x0->d || pred->d == dist->d))))
    return fail(e, SH_EINVAL, "sh_sssp: dist and pred must not alias x0 or each other");
  if (delta <= 0) delta = g->delta > 0 ? g->delta : 1.0;
  *rounds = 0; *buckets = 0; *reached = 0; *complete = 1; *relaxed = 0;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, SSSP_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  uint32_t *d = (uint32_t *)dist->d;
  uint64_t total = 0, ns = 0;
  // dist and the stamps from x0, the sources as far list 0
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, SSSP_CTL_BYTES, e->stream));
  hipLaunchKernelGGL(sssp_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, (const uint32_t *)x0->d, d, g->d_stamp, g->d_far[0]);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(sssp_decide, dim3(1), block, 0, e->stream, g->d_ctl, 0, -1, nblocks, g->d_part);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the four launches of a round: each returns at once unless the control block says the round runs (with a split)
  const auto enqueue = [&](int R, int k) {
    const int p = R & 1;
    for (int phase = 0; phase < 2; phase++) {
      hipLaunchKernelGGL(sssp_split, grid, block, 0, e->stream, g->d_ctl, R, phase, nblocks, delta, g->d_pmin, d, g->d_stamp,
                         g->d_out_ptr, g->d_far[0], g->d_far[1], g->d_near[p], g->d_opieces[p]);
      HIP_TRY(e, hipGetLastError());
    }
    hipLaunchKernelGGL(sssp_relax, grid, block, 0, e->stream, g->d_ctl, R, d, g->d_stamp, g->d_out_ptr, g->d_out_row, g->d_out_w,
                       g->d_near[p], g->d_opieces[p], g->d_near[p ^ 1], g->d_opieces[p ^ 1], g->d_far[0], g->d_far[1], g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(sssp_decide, dim3(1), block, 0, e->stream, g->d_ctl, k, R, nblocks, g->d_part);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int R, const SsspRec &rc, uint64_t round_ns) {
    if (ns_per_round) ns_per_round[R] = round_ns;
    if (size_per_round) size_per_round[R] = (int64_t)rc.size;
    if (edges_per_round) edges_per_round[R] = (int64_t)rc.edges;
  };
  const int rc = run_batches(e, "sh_sssp: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  if (pred && done) {
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    HIP_TRY(e, hipMemsetAsync(pred->d, 0xFF, (size_t)rows * 4, e->stream));
    hipLaunchKernelGGL(sssp_preds, grid, block, 0, e->stream, (int32_t)rows, (const uint32_t *)x0->d, (const uint32_t *)d, g->d_in_ptr,
                       g->d_in_col, g->d_in_w, g->d_rpieces, g->n_rpieces, (int32_t *)pred->d);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
    total += ns;
  }
  *rounds = it;
  *buckets = (int32_t)g->h_ctl->buckets;
  *reached = (int64_t)g->h_ctl->reached;
  *relaxed = (int64_t)g->h_ctl->relaxed;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- strongly connected components by trim, pivot and colouring (scc.hip.h) ------------------------------------------
struct sh_scc_graph : GraphHandle<SccCtl> {   // d_ctl: SCC_CTL_BYTES, followed by the WlParts and the pivot candidates
  uint32_t *d_colour = nullptr, *d_stamp = nullptr, *d_list[2] = {nullptr, nullptr}, *d_cand = nullptr;
  WlPiece *d_opieces[2] = {nullptr, nullptr}, *d_ipieces[2] = {nullptr, nullptr};   // pieces of the long out- / in-lists of list 0 / 1
  SccPick *d_pick = nullptr;
};
static_assert(sizeof(SccCtl) <= SCC_CTL_BYTES, "the control block is accounted as SCC_CTL_BYTES (sh_scc_graph_footprint)");
static_assert(sizeof(WlPart) * SCC_MAX_BLOCKS == SCC_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(SccPick) * SCC_MAX_BLOCKS == SCC_PICK_BYTES, "one SccPick per workgroup");

extern "C" {

int sh_scc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_scc_graph **out) {
  return create_graph_handle<sh_scc_graph>(e, "sh_scc_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_scc_graph *g) -> int {
    int rc;
    if ((rc = build_edge_lists<BfsKeep, SCC_ROW_PIECE>(e, g, rows, nnz, row_ptr, col_idx, val, false)))
      return rc;
    const int64_t E = g->edges;
    HIP_TRY(e, g->dev.alloc(&g->d_colour, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->d_stamp, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->d_cand, rows * 4));
    for (int i = 0; i < 2; i++) {
      HIP_TRY(e, g->dev.alloc(&g->d_list[i], rows * 4));
      HIP_TRY(e, g->dev.alloc(&g->d_opieces[i], (E / 1024 + 1) * sizeof(WlPiece)));   // see wl_push_pieces: lists longer than 2048
      HIP_TRY(e, g->dev.alloc(&g->d_ipieces[i], (E / 1024 + 1) * sizeof(WlPiece)));
    }
    if ((rc = open_control(e, g, SCC_CTL_BYTES, SCC_CTL_BYTES + SCC_PART_BYTES + SCC_PICK_BYTES)))
      return rc;
    g->d_pick = (SccPick *)((char *)g->d_ctl + SCC_CTL_BYTES + SCC_PART_BYTES);
    return SH_OK;
  });
}

int sh_scc_graph_free(sh_engine *e, sh_scc_graph *g) { return free_handle(e, g); }

int sh_scc_graph_footprint(const sh_scc_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_scc_graph_edges(const sh_scc_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_scc(sh_engine *e, sh_scc_graph *g, sh_vec *comp, int32_t trim, int32_t pivot, int32_t max_steps,
           int64_t *components, int64_t *settled, int64_t *trimmed, int32_t *rounds, int32_t *steps, int32_t *complete,
           int32_t *kind_per_round, int64_t *size_per_round, int32_t *steps_per_round, int64_t *edges_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (max_steps < 1)
    return fail(e, SH_EINVAL, "sh_scc: max_steps = %d, must be at least 1", (int)max_steps);
  if (!e || !g || !comp || !components || !settled || !trimmed || !rounds || !steps || !complete)
    return fail(e, SH_EINVAL, "sh_scc: NULL argument (engine, graph, comp, components, settled, trimmed, rounds, steps or complete)");
  const int64_t rows = g->rows;
  if (comp->n < rows)
    return fail(e, SH_ESHAPE, "sh_scc: comp is shorter than the graph's %lld rows", (long long)rows);
  *components = 0; *settled = 0; *trimmed = 0; *rounds = 0; *steps = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, SCC_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const SccGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col, g->d_out_ptr, g->d_out_row};
  const SccLists L{g->d_list[0], g->d_list[1], g->d_cand, g->d_opieces[0], g->d_opieces[1], g->d_ipieces[0], g->d_ipieces[1]};
  int32_t *c = (int32_t *)comp->d;
  uint64_t total = 0;
  // every vertex live, the stamps cleared, the first phase chosen
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, SCC_CTL_BYTES, e->stream));
  hipLaunchKernelGGL(scc_init, grid, block, 0, e->stream, (int32_t)rows, c, g->d_stamp);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(scc_decide, dim3(1), block, 0, e->stream, g->d_ctl, 0, -1, nblocks, g->d_part, (int32_t)rows, trim != 0 ? 1 : 0,
                     pivot != 0 ? 1 : 0);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0, n_rounds = 0;
  bool done = false;
  // the eight launches of a step: each returns at once unless the control block says the step is in its phase
  const auto enqueue = [&](int s, int k) {
    for (int phase = 0; phase < 2; phase++) {
      hipLaunchKernelGGL(scc_trim, grid, block, 0, e->stream, g->d_ctl, s, phase, G, L, c, g->d_stamp, g->d_part);
      HIP_TRY(e, hipGetLastError());
    }
    hipLaunchKernelGGL(scc_pick, grid, block, 0, e->stream, g->d_ctl, s, G, c, g->d_pick);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(scc_seed, grid, block, 0, e->stream, g->d_ctl, s, nblocks, G, L, c, g->d_colour, g->d_pick);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(scc_propagate, grid, block, 0, e->stream, g->d_ctl, s, G, L, c, g->d_colour, g->d_stamp, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(scc_claim, grid, block, 0, e->stream, g->d_ctl, s, G, L, c, g->d_colour, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(scc_label, grid, block, 0, e->stream, g->d_ctl, s, (int32_t)rows, c, g->d_colour, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(scc_decide, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part, (int32_t)rows, 0, 0);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  // the steps of one round add up; a round that settled nothing (a trim round that found nothing to trim) is not recorded
  struct { int32_t id = -1, kind = 0, steps = 0; int64_t size = 0, edges = 0; uint64_t ns = 0; } cur;
  const auto flush = [&]() {
    if (cur.id >= 0 && cur.size > 0) {
      if (kind_per_round) kind_per_round[n_rounds] = cur.kind;
      if (size_per_round) size_per_round[n_rounds] = cur.size;
      if (steps_per_round) steps_per_round[n_rounds] = cur.steps;
      if (edges_per_round) edges_per_round[n_rounds] = cur.edges;
      if (ns_per_round) ns_per_round[n_rounds] = cur.ns;
      n_rounds++;
    }
  };
  const auto take = [&](int, const SccRec &rc, uint64_t step_ns) {
    if (rc.round != cur.id) {
      flush();
      cur.id = rc.round; cur.kind = rc.kind; cur.steps = 0; cur.size = 0; cur.edges = 0; cur.ns = 0;
    }
    cur.steps++; cur.size += (int64_t)rc.settled; cur.edges += (int64_t)rc.edges; cur.ns += step_ns;
  };
  const int rc = run_batches(e, "sh_scc: step", g, max_steps, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  flush();
  *components = (int64_t)g->h_ctl->components;
  *settled = (int64_t)g->h_ctl->settled;
  *trimmed = (int64_t)g->h_ctl->trimmed;
  *rounds = n_rounds;
  *steps = it;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- weakly connected components by hooking roots and pointer jumping (wcc.hip.h) ------------------------------------
struct sh_wcc_graph : GraphHandle<WccCtl> {   // d_ctl: WCC_CTL_BYTES, followed by the WlParts of the walk and those of the jumps
  uint32_t *d_parent = nullptr, *d_list = nullptr;
  WlPiece *d_ipieces = nullptr, *d_opieces = nullptr;   // pieces of the long in- / out-lists of the work list's vertices
  WlPart *d_jpart = nullptr;
};
static_assert(sizeof(WccCtl) <= WCC_CTL_BYTES, "the control block is accounted as WCC_CTL_BYTES (sh_wcc_graph_footprint)");
static_assert(sizeof(WlPart) * WCC_MAX_BLOCKS == WCC_PART_BYTES, "one WlPart per workgroup");

extern "C" {

int sh_wcc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_wcc_graph **out) {
  return create_graph_handle<sh_wcc_graph>(e, "sh_wcc_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_wcc_graph *g) -> int {
    int rc;
    if ((rc = build_edge_lists<BfsKeep, WCC_ROW_PIECE>(e, g, rows, nnz, row_ptr, col_idx, val, false)))
      return rc;
    const int64_t E = g->edges;
    HIP_TRY(e, g->dev.alloc(&g->d_parent, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->d_list, rows * 4));   // a vertex joins the work list at most once per call (wcc_compact)
    HIP_TRY(e, g->dev.alloc(&g->d_ipieces, (E / (WCC_PIECE / 2) + 1) * sizeof(WlPiece)));   // see wl_push_pieces
    HIP_TRY(e, g->dev.alloc(&g->d_opieces, (E / (WCC_PIECE / 2) + 1) * sizeof(WlPiece)));
    if ((rc = open_control(e, g, WCC_CTL_BYTES, WCC_CTL_BYTES + 2 * WCC_PART_BYTES)))
      return rc;
    g->d_jpart = (WlPart *)((char *)g->d_ctl + WCC_CTL_BYTES + WCC_PART_BYTES);
    return SH_OK;
  });
}

int sh_wcc_graph_free(sh_engine *e, sh_wcc_graph *g) { return free_handle(e, g); }

int sh_wcc_graph_footprint(const sh_wcc_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_wcc_graph_edges(const sh_wcc_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_wcc(sh_engine *e, sh_wcc_graph *g, sh_vec *comp, int32_t sample, int32_t max_rounds,
           int64_t *components, int64_t *skipped, int32_t *rounds, int32_t *complete,
           int32_t *kind_per_round, int64_t *hooks_per_round, int64_t *jumps_per_round, int64_t *edges_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (sample < 0)
    return fail(e, SH_EINVAL, "sh_wcc: sample = %d, must not be negative", (int)sample);
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_wcc: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (!e || !g || !comp || !components || !skipped || !rounds || !complete)
    return fail(e, SH_EINVAL, "sh_wcc: NULL argument (engine, graph, comp, components, skipped, rounds or complete)");
  const int64_t rows = g->rows;
  if (comp->n < rows)
    return fail(e, SH_ESHAPE, "sh_wcc: comp is shorter than the graph's %lld rows", (long long)rows);
  *components = 0; *skipped = 0; *rounds = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, WCC_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const WccGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col, g->d_out_ptr, g->d_out_row};
  uint32_t *p = g->d_parent;
  uint64_t total = 0, ns = 0;
  // every vertex a tree of its own
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, WCC_CTL_BYTES, e->stream));
  hipLaunchKernelGGL(wcc_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, sample, p);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its kind (and, for a
  // jumping launch after the first, unless the one before it changed a pointer)
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(wcc_sample, grid, block, 0, e->stream, g->d_ctl, s, G, p, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wcc_compact, grid, block, 0, e->stream, g->d_ctl, s, G, p, g->d_list, g->d_ipieces, g->d_opieces);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wcc_full, grid, block, 0, e->stream, g->d_ctl, s, G, p, g->d_list, g->d_ipieces, g->d_opieces, g->d_part);
    HIP_TRY(e, hipGetLastError());
    for (int i = 0; i < WCC_SWEEPS; i++) {
      hipLaunchKernelGGL(wcc_jump, grid, block, 0, e->stream, g->d_ctl, s, i, (int32_t)rows, p, g->d_jpart);
      HIP_TRY(e, hipGetLastError());
    }
    hipLaunchKernelGGL(wcc_decide, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part, g->d_jpart);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const WccRec &rc, uint64_t round_ns) {
    if (kind_per_round) kind_per_round[s] = rc.kind;
    if (hooks_per_round) hooks_per_round[s] = (int64_t)rc.hooks;
    if (jumps_per_round) jumps_per_round[s] = (int64_t)rc.jumps;
    if (edges_per_round) edges_per_round[s] = (int64_t)rc.edges;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_wcc: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // the labels (or -1 everywhere) and the number of roots
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  hipLaunchKernelGGL(wcc_label, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, done ? 1 : 0, p, (int32_t *)comp->d);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  HIP_TRY(e, hipMemcpyAsync(g->h_ctl, g->d_ctl, sizeof(WccCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  total += ns;
  *components = (int64_t)g->h_ctl->components;
  *skipped = (int64_t)g->h_ctl->skipped;
  *rounds = it;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- triangle counts by intersecting forward lists (tri.hip.h) -------------------------------------------------------
// (a GraphBase, not a GraphHandle: sh_tri is a fixed handful of launches, so it needs neither the pinned copy of a control
// block nor the events of a batch)
struct sh_tri_graph : GraphBase {   // d_ctl: TRI_CTL_BYTES, followed by the TriParts of tri_count_light and those of tri_count_heavy
  int64_t max_forward = 0;
  int32_t *d_fwd_ptr = nullptr, *d_fwd_col = nullptr;
  uint32_t *d_deg = nullptr;
  TriCtl *d_ctl = nullptr;
  TriPart *d_part = nullptr;
};
static_assert(sizeof(TriCtl) <= TRI_CTL_BYTES, "the control block is accounted as TRI_CTL_BYTES (sh_tri_graph_footprint)");
static_assert(sizeof(TriPart) * TRI_MAX_BLOCKS == TRI_PART_BYTES, "one TriPart per workgroup");

// What the builds of sh_tri_graph and sh_core_graph share: the edges of the simple undirected graph under host CSR arrays.
// The entries that count and are no self-loops become keys (min << bits | max), sorted; the first key of every run is an
// edge; deg (zeroed by the caller) is the histogram over both ends.  Leaves in `tmp`: sorted[S] with head[S + 1] and its
// exclusive scan pos[S + 1] (edge i of the M stands at the key with head = 1 and pos = i), and key[S] free for reuse.
struct UndEdges {
  int64_t S = 0, M = 0;   // surviving entries, edges of the simple graph
  int bits = 1;           // of the largest index
  uint64_t *key = nullptr, *sorted = nullptr;
  uint32_t *head = nullptr, *pos = nullptr;
  const int32_t *rp = nullptr, *ci = nullptr;   // the device copies of the arrays as given (NULL without entries), for
  const uint32_t *val = nullptr;                // sh_msf_graph_create's pass over the values
};
static int build_und_edges(sh_engine *e, DevArrays &tmp, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                           const void *val, uint32_t *deg, UndEdges *u) {
  // temporaries: the CSR arrays as given, flags and their scan (twice), the keys and the sorted keys
  int32_t *t_rp = nullptr, *t_ci = nullptr;
  uint32_t *t_val = nullptr, *t_flag = nullptr, *t_pos = nullptr;
  uint64_t *t_key = nullptr, *t_sorted = nullptr;
  int64_t S = 0, M = 0;
  const int bits = 32 - __builtin_clz((unsigned)std::max<int64_t>(rows - 1, 1));   // (rows <= 2^31 - 256)
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  if (rows > 0 && nnz > 0) {
    HIP_TRY(e, tmp.alloc(&t_rp, (rows + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_ci, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_val, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_flag, (nnz + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_pos, (nnz + 1) * 4));
    HIP_TRY(e, hipMemcpyAsync(t_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wl_und_flag<BfsKeep>), grid_for(nnz + 1), blk, 0, e->stream, t_rp, t_ci, t_val, nnz, (int32_t)rows, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, nnz + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + nnz, 4, hipMemcpyDeviceToHost));
    S = (int64_t)n;
  }
  if (S > 0) {
    HIP_TRY(e, tmp.alloc(&t_key, S * 8));
    HIP_TRY(e, tmp.alloc(&t_sorted, S * 8));
    hipLaunchKernelGGL(wl_und_keys, grid_for(nnz), blk, 0, e->stream, t_rp, t_ci, t_flag, t_pos, nnz, (int32_t)rows, bits, t_key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_key, t_sorted, S, 2 * bits));
    // (t_flag and t_pos hold nnz + 1 >= S + 1 words: they serve the run heads and their scan)
    hipLaunchKernelGGL(wl_run_heads, grid_for(S + 1), blk, 0, e->stream, t_sorted, S, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, S + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + S, 4, hipMemcpyDeviceToHost));
    M = (int64_t)n;
  }
  if (M > 0) {
    hipLaunchKernelGGL(wl_und_degrees, grid_for(S), blk, 0, e->stream, t_sorted, t_flag, S, bits, deg);
    HIP_TRY(e, hipGetLastError());
  }
  *u = UndEdges{S, M, bits, t_key, t_sorted, t_flag, t_pos, t_rp, t_ci, t_val};
  return SH_OK;
}

// The forward lists of a triangle handle from host CSR arrays: the edges of the simple graph and the degrees
// (build_und_edges), the oriented keys sorted again.  Returns with the stream synchronised: the host arrays are done with.
static int build_forward_lists(sh_engine *e, sh_tri_graph *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                               const void *val, int32_t order) {
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  HIP_TRY(e, own.alloc(&g->d_fwd_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_deg, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_ctl, TRI_CTL_BYTES + 2 * TRI_PART_BYTES));
  g->d_part = (TriPart *)((char *)g->d_ctl + TRI_CTL_BYTES);
  HIP_TRY(e, hipMemsetAsync(g->d_fwd_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_deg, 0, (size_t)std::max<int64_t>(rows, 1) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, TRI_CTL_BYTES + 2 * TRI_PART_BYTES, e->stream));
  DevArrays tmp;
  UndEdges u;
  const int rc = build_und_edges(e, tmp, rows, nnz, row_ptr, col_idx, val, g->d_deg, &u);
  if (rc)
    return rc;
  const int64_t S = u.S, M = u.M;
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  g->edges = M;
  HIP_TRY(e, own.alloc(&g->d_fwd_col, M * 4));
  if (M > 0) {
    hipLaunchKernelGGL(wl_orient, grid_for(S), blk, 0, e->stream, u.sorted, u.head, u.pos, S, u.bits, order, g->d_deg, u.key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, u.key, u.sorted, M, 2 * u.bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(M, rows + 1)), blk, 0, e->stream, u.sorted, M, rows, u.bits, g->d_fwd_ptr, g->d_fwd_col);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wl_max_len, dim3((unsigned)std::max(1, std::min(e->n_cus * 4, TRI_MAX_BLOCKS))), blk, 0, e->stream, g->d_fwd_ptr, rows,
                       &g->d_ctl->max_forward);
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t longest = 0;
  HIP_TRY(e, hipMemcpyAsync(&longest, &g->d_ctl->max_forward, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->max_forward = (int64_t)longest;
  return SH_OK;
}

template <bool PER_VERTEX>
static void launch_tri(sh_engine *e, sh_tri_graph *g, dim3 grid, uint64_t *tri) {
  const dim3 block(WL_BS);
  const TriGraph G{(int32_t)g->rows, g->d_fwd_ptr, g->d_fwd_col};
  hipLaunchKernelGGL(HIP_KERNEL_NAME(tri_count_light<PER_VERTEX>), grid, block, 0, e->stream, G, tri, g->d_part);
  if (g->max_forward > TRI_WAVE)   // (a fact of the handle, known since it was built: not a host loop)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(tri_count_heavy<PER_VERTEX>), grid, block, 0, e->stream, G, tri, g->d_part + TRI_MAX_BLOCKS);
}

extern "C" {

int sh_tri_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, int32_t order, sh_tri_graph **out) {
  if (out) *out = nullptr;
  if (order != 0 && order != 1)   // (what the scalar alone decides comes before what the arrays do)
    return fail(e, SH_EINVAL, "sh_tri_graph_create: order = %d, must be 0 (by index) or 1 (by degree, then index)", (int)order);
  return create_graph_handle<sh_tri_graph>(e, "sh_tri_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_tri_graph *g) -> int {
    return build_forward_lists(e, g, rows, nnz, row_ptr, col_idx, val, order);
  });
}

int sh_tri_graph_free(sh_engine *e, sh_tri_graph *g) { return free_handle(e, g); }

int sh_tri_graph_footprint(const sh_tri_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_tri_graph_edges(const sh_tri_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_tri_graph_max_forward(const sh_tri_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_forward); }

int sh_tri(sh_engine *e, sh_tri_graph *g, sh_vec *tri, sh_vec *deg, uint64_t *triangles, uint64_t *probes, uint64_t *total_ns) {
  if (!e || !g || !triangles)
    return fail(e, SH_EINVAL, "sh_tri: NULL argument (engine, graph or triangles)");
  const int64_t rows = g->rows;
  if (tri && tri->n < 2 * rows)
    return fail(e, SH_ESHAPE, "sh_tri: tri holds fewer than 2 elements for each of the graph's %lld rows", (long long)rows);
  if (deg && deg->n < rows)
    return fail(e, SH_ESHAPE, "sh_tri: deg is shorter than the graph's %lld rows", (long long)rows);
  if (tri && ((uintptr_t)tri->d & 7u))
    return fail(e, SH_EINVAL, "sh_tri: tri is not aligned to 8 bytes");
  *triangles = 0;
  if (probes) *probes = 0;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const dim3 grid((unsigned)std::max(1, std::min(e->n_cus * 4, TRI_MAX_BLOCKS)));
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  // (the TriParts of a launch that does not run stay zero)
  HIP_TRY(e, hipMemsetAsync(g->d_part, 0, 2 * TRI_PART_BYTES, e->stream));
  if (tri) HIP_TRY(e, hipMemsetAsync(tri->d, 0, (size_t)rows * 8, e->stream));
  if (deg) HIP_TRY(e, hipMemcpyAsync(deg->d, g->d_deg, (size_t)rows * 4, hipMemcpyDeviceToDevice, e->stream));
  if (tri) launch_tri<true>(e, g, grid, (uint64_t *)tri->d);
  else launch_tri<false>(e, g, grid, nullptr);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(tri_finish, dim3(1), dim3(WL_BS), 0, e->stream, g->d_ctl, 2 * TRI_MAX_BLOCKS, g->d_part);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  TriCtl got;
  HIP_TRY(e, hipMemcpyAsync(&got, g->d_ctl, sizeof(TriCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  uint64_t ns = 0;
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  *triangles = got.triangles;
  if (probes) *probes = got.probes;
  if (total_ns) *total_ns = ns;
  return SH_OK;
}

} // extern "C"

// ---- core numbers by parallel peeling (core.hip.h) -------------------------------------------------------------------
// The GraphHandle base serves run_batches (control block, pinned copy, events).  Of its edge arrays the symmetric lists
// use d_in_ptr / d_in_col alone (adj_ptr / adj_col): a list is its own transpose, so d_out_* and the static row pieces
// stay NULL and take no memory.  d_ctl: CORE_CTL_BYTES, followed by the WlParts of core_peel and those of core_min.
struct sh_core_graph : GraphHandle<CoreCtl> {
  int64_t max_degree = 0;
  uint32_t *d_deg = nullptr;
  int32_t *d_cur = nullptr;
  CoreLists lists = {};
  WlPart *d_mins = nullptr;
};
static_assert(sizeof(CoreCtl) <= CORE_CTL_BYTES, "the control block is accounted as CORE_CTL_BYTES (sh_core_graph_footprint)");
static_assert(sizeof(WlPart) * CORE_MAX_BLOCKS == CORE_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(CoreCtl::rec) / sizeof(CoreRec) == CORE_BATCH, "one record per round of a batch");

// The symmetric lists of a core or truss handle (fn = sh_core_graph_create / sh_truss_graph_create) from host CSR arrays:
// the edges of the simple graph and the degrees (build_und_edges), every edge as two keys (src << bits | dst), sorted,
// the row starts taken from them.  ptr, col and deg are the handle's (`own`); `tmp` keeps what build_und_edges left (u)
// until the caller lets go of it.  Returns with the stream synchronised: the host arrays are done with.
struct SymLists {
  int32_t *ptr = nullptr, *col = nullptr;
  uint32_t *deg = nullptr;
  int64_t max_degree = 0;
  UndEdges u;
};
static int build_symmetric_lists(sh_engine *e, const char *fn, DevArrays &own, DevArrays &tmp, int64_t rows, int64_t nnz,
                                 const int32_t *row_ptr, const int32_t *col_idx, const void *val, SymLists *out) {
  SymLists &g = *out;
  HIP_TRY(e, own.alloc(&g.ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g.deg, rows * 4));
  HIP_TRY(e, hipMemsetAsync(g.ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(g.deg, 0, (size_t)std::max<int64_t>(rows, 1) * 4, e->stream));
  UndEdges &u = g.u;
  const int rc = build_und_edges(e, tmp, rows, nnz, row_ptr, col_idx, val, g.deg, &u);
  if (rc)
    return rc;
  const int64_t S = u.S, M = u.M, E = 2 * M;
  if (E > 0x7FFFFF00ll)
    return fail(e, SH_EINVAL, "%s: the lists hold %lld entries (twice the %lld edges), must be at most 2^31 - 256", fn,
                (long long)E, (long long)M);
  HIP_TRY(e, own.alloc(&g.col, E * 4));
  uint32_t *t_longest = nullptr;
  HIP_TRY(e, tmp.alloc(&t_longest, 4));
  HIP_TRY(e, hipMemsetAsync(t_longest, 0, 4, e->stream));
  if (M > 0) {
    const dim3 blk(WL_BS);
    const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
    uint64_t *t_key = nullptr, *t_sorted = nullptr;
    HIP_TRY(e, tmp.alloc(&t_key, E * 8));
    HIP_TRY(e, tmp.alloc(&t_sorted, E * 8));
    hipLaunchKernelGGL(wl_both_ways, grid_for(S), blk, 0, e->stream, u.sorted, u.head, u.pos, S, u.bits, t_key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_key, t_sorted, E, 2 * u.bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(E, rows + 1)), blk, 0, e->stream, t_sorted, E, rows, u.bits, g.ptr, g.col);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wl_max_len, dim3((unsigned)std::max(1, std::min(e->n_cus * 4, CORE_MAX_BLOCKS))), blk, 0, e->stream, g.ptr, rows,
                       t_longest);
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t longest = 0;
  HIP_TRY(e, hipMemcpyAsync(&longest, t_longest, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g.max_degree = (int64_t)longest;
  return SH_OK;
}

extern "C" {

int sh_core_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                         const void *val, sh_core_graph **out) {
  return create_graph_handle<sh_core_graph>(e, "sh_core_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_core_graph *g) -> int {
    int rc;
    g->rows = rows; g->nnz = nnz;
    SymLists s;
    {
      DevArrays tmp;
      if ((rc = build_symmetric_lists(e, "sh_core_graph_create", g->dev, tmp, rows, nnz, row_ptr, col_idx, val, &s)))
        return rc;
    }
    g->d_in_ptr = s.ptr; g->d_in_col = s.col; g->d_deg = s.deg;
    g->edges = s.u.M; g->max_degree = s.max_degree;
    HIP_TRY(e, g->dev.alloc(&g->d_cur, rows * 4));
    for (int i = 0; i < 2; i++) {
      HIP_TRY(e, g->dev.alloc(&g->lists.list[i], rows * 4));   // a vertex joins a work list at most once per call (core.hip.h, invariant 1)
      HIP_TRY(e, g->dev.alloc(&g->lists.pieces[i], (2 * s.u.M / (CORE_PIECE / 2) + 1) * sizeof(WlPiece)));   // see wl_push_pieces
    }
    if ((rc = open_control(e, g, CORE_CTL_BYTES, CORE_CTL_BYTES + 2 * CORE_PART_BYTES)))
      return rc;
    g->d_mins = (WlPart *)((char *)g->d_ctl + CORE_CTL_BYTES + CORE_PART_BYTES);
    return SH_OK;
  });
}

int sh_core_graph_free(sh_engine *e, sh_core_graph *g) { return free_handle(e, g); }

int sh_core_graph_footprint(const sh_core_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_core_graph_edges(const sh_core_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_core_graph_max_degree(const sh_core_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_degree); }

int sh_core(sh_engine *e, sh_core_graph *g, sh_vec *core, sh_vec *deg, int32_t chase, int32_t max_rounds,
            int32_t *degeneracy, int32_t *levels, int32_t *rounds, int32_t *complete,
            int32_t *k_per_round, int64_t *size_per_round, int64_t *chased_per_round, int64_t *edges_per_round,
            uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (chase < 0)
    return fail(e, SH_EINVAL, "sh_core: chase = %d, must not be negative", (int)chase);
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_core: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (!e || !g || !core || !degeneracy || !levels || !rounds || !complete)
    return fail(e, SH_EINVAL, "sh_core: NULL argument (engine, graph, core, degeneracy, levels, rounds or complete)");
  const int64_t rows = g->rows;
  if (core->n < rows)
    return fail(e, SH_ESHAPE, "sh_core: core is shorter than the graph's %lld rows", (long long)rows);
  if (deg && deg->n < rows)
    return fail(e, SH_ESHAPE, "sh_core: deg is shorter than the graph's %lld rows", (long long)rows);
  *degeneracy = 0; *levels = 0; *rounds = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, CORE_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const CoreGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col};
  int32_t *c = (int32_t *)core->d;
  uint64_t total = 0;
  // every vertex unsettled, its remaining degree its degree
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, CORE_CTL_BYTES, e->stream));
  if (deg) HIP_TRY(e, hipMemcpyAsync(deg->d, g->d_deg, (size_t)rows * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(core_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, chase, g->d_deg, g->d_cur, c);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its turn (and, for the
  // two passes that open a level, unless the work list is empty)
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(core_min, grid, block, 0, e->stream, g->d_ctl, s, (int32_t)rows, g->d_cur, c, g->d_mins);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(core_open, grid, block, 0, e->stream, g->d_ctl, s, G, g->d_cur, c, g->d_mins, g->lists);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(core_peel, grid, block, 0, e->stream, g->d_ctl, s, G, g->d_cur, c, g->lists, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(core_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const CoreRec &rc, uint64_t round_ns) {
    if (k_per_round) k_per_round[s] = rc.k;
    if (size_per_round) size_per_round[s] = (int64_t)rc.size;
    if (chased_per_round) chased_per_round[s] = (int64_t)rc.chased;
    if (edges_per_round) edges_per_round[s] = (int64_t)rc.edges;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_core: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // (the control block as the last batch's readback left it in h_ctl: levels and the latest of them)
  *degeneracy = g->h_ctl->degeneracy;
  *levels = g->h_ctl->levels;
  *rounds = it;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- truss numbers by parallel peeling (truss.hip.h) -----------------------------------------------------------------
// The GraphHandle base serves run_batches (control block, pinned copy, events).  As in sh_core_graph the symmetric lists
// use d_in_ptr / d_in_col alone (adj_ptr / adj_col).  d_ctl: TRUSS_CTL_BYTES, followed by the TrussParts of truss_peel,
// the WlParts of truss_min and the TrussParts of truss_support.
struct sh_truss_graph : GraphHandle<TrussCtl> {
  int64_t max_degree = 0;
  uint32_t *d_deg = nullptr;
  int32_t *d_eid = nullptr, *d_eu = nullptr, *d_ev = nullptr, *d_sup = nullptr, *d_stamp = nullptr;
  TrussLists lists = {};
  WlPart *d_mins = nullptr;
  TrussPart *d_sparts = nullptr;
};
static_assert(sizeof(TrussCtl) <= TRUSS_CTL_BYTES, "the control block is accounted as TRUSS_CTL_BYTES (sh_truss_graph_footprint)");
static_assert(sizeof(TrussPart) * TRUSS_MAX_BLOCKS == TRUSS_PART_BYTES && sizeof(WlPart) == sizeof(TrussPart), "one part per workgroup");
static_assert(sizeof(TrussCtl::rec) / sizeof(TrussRec) == TRUSS_BATCH, "one record per round of a batch");

extern "C" {

int sh_truss_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_truss_graph **out) {
  return create_graph_handle<sh_truss_graph>(e, "sh_truss_graph_create", rows, nnz, row_ptr, col_idx, val, out, [&](sh_truss_graph *g) -> int {
    int rc;
    g->rows = rows; g->nnz = nnz;
    DevArrays &own = g->dev;
    DevArrays tmp;   // (what build_und_edges left: the sorted keys, their run heads and the scan of those)
    SymLists s;
    if ((rc = build_symmetric_lists(e, "sh_truss_graph_create", own, tmp, rows, nnz, row_ptr, col_idx, val, &s)))
      return rc;
    const int64_t M = s.u.M;
    g->d_in_ptr = s.ptr; g->d_in_col = s.col; g->d_deg = s.deg;
    g->edges = M; g->max_degree = s.max_degree;
    HIP_TRY(e, own.alloc(&g->d_eid, 2 * M * 4));
    HIP_TRY(e, own.alloc(&g->d_eu, M * 4));
    HIP_TRY(e, own.alloc(&g->d_ev, M * 4));
    HIP_TRY(e, own.alloc(&g->d_sup, M * 4));
    HIP_TRY(e, own.alloc(&g->d_stamp, M * 4));
    for (int i = 0; i < 2; i++)
      HIP_TRY(e, own.alloc(&g->lists.list[i], M * 4));   // an edge joins a work list at most once per call (truss.hip.h, invariant 1)
    if (M > 0) {
      const dim3 blk(WL_BS);
      const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
      hipLaunchKernelGGL(wl_edge_ends, grid_for(s.u.S), blk, 0, e->stream, s.u.sorted, s.u.head, s.u.pos, s.u.S, s.u.bits, g->d_eu, g->d_ev);
      HIP_TRY(e, hipGetLastError());
      hipLaunchKernelGGL(wl_edge_ids, grid_for(2 * M), blk, 0, e->stream, g->d_in_ptr, g->d_in_col, 2 * M, (int32_t)rows, g->d_eu, g->d_ev, M,
                         g->d_eid);
      HIP_TRY(e, hipGetLastError());
    }
    if ((rc = open_control(e, g, TRUSS_CTL_BYTES, TRUSS_CTL_BYTES + 3 * TRUSS_PART_BYTES)))
      return rc;
    g->d_mins = (WlPart *)((char *)g->d_ctl + TRUSS_CTL_BYTES + TRUSS_PART_BYTES);
    g->d_sparts = (TrussPart *)((char *)g->d_ctl + TRUSS_CTL_BYTES + 2 * TRUSS_PART_BYTES);
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // (the kernels above read `tmp`)
    return SH_OK;
  });
}

int sh_truss_graph_free(sh_engine *e, sh_truss_graph *g) { return free_handle(e, g); }

int sh_truss_graph_footprint(const sh_truss_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_truss_graph_edges(const sh_truss_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_truss_graph_max_degree(const sh_truss_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_degree); }

int sh_truss(sh_engine *e, sh_truss_graph *g, sh_vec *truss, sh_vec *support, sh_vec *edge_u, sh_vec *edge_v, int32_t max_rounds,
             int32_t *max_truss, int32_t *levels, int32_t *rounds, int32_t *complete, uint64_t *triangles,
             int32_t *k_per_round, int64_t *size_per_round, int64_t *walked_per_round, uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalar alone decides comes first: no handle is needed to be told
  if (max_rounds < 0)
    return fail(e, SH_EINVAL, "sh_truss: max_rounds = %d, must not be negative", (int)max_rounds);
  if (!e || !g || !truss || !max_truss || !levels || !rounds || !complete || !triangles)
    return fail(e, SH_EINVAL, "sh_truss: NULL argument (engine, graph, truss, max_truss, levels, rounds, complete or triangles)");
  const int64_t M = g->edges;
  const struct { const sh_vec *v; const char *name; } vecs[] = {{truss, "truss"}, {support, "support"}, {edge_u, "edge_u"}, {edge_v, "edge_v"}};
  for (const auto &x : vecs)
    if (x.v && x.v->n < M)
      return fail(e, SH_ESHAPE, "sh_truss: %s is shorter than the graph's %lld edges", x.name, (long long)M);
  *max_truss = 0; *levels = 0; *rounds = 0; *complete = 1; *triangles = 0;
  if (total_ns) *total_ns = 0;
  if (M == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, TRUSS_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const TrussGraph G{(int32_t)g->rows, (int32_t)M, g->d_in_ptr, g->d_in_col, g->d_eid, g->d_eu, g->d_ev};
  int32_t *t = (int32_t *)truss->d;
  uint64_t total = 0;
  // every edge alive and unsettled, its remaining support its support
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, TRUSS_CTL_BYTES, e->stream));
  if (edge_u) HIP_TRY(e, hipMemcpyAsync(edge_u->d, g->d_eu, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  if (edge_v) HIP_TRY(e, hipMemcpyAsync(edge_v->d, g->d_ev, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  uint32_t *far1 = g->lists.list[1] + (M - 1);   // (list 1 is empty until round 1 fills it: its far end lends itself)
  hipLaunchKernelGGL(truss_init, grid, block, 0, e->stream, g->d_ctl, G, g->d_sup, g->d_stamp, t, far1);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(truss_support, grid, block, 0, e->stream, g->d_ctl, G, g->d_sup, far1, g->d_sparts);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(truss_total, dim3(1), block, 0, e->stream, g->d_ctl, nblocks, g->d_sparts);
  HIP_TRY(e, hipGetLastError());
  if (support) HIP_TRY(e, hipMemcpyAsync(support->d, g->d_sup, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its turn (and, for the
  // two passes that open a level, unless the work list is empty)
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(truss_min, grid, block, 0, e->stream, g->d_ctl, s, (int32_t)M, g->d_sup, g->d_stamp, g->d_mins);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(truss_open, grid, block, 0, e->stream, g->d_ctl, s, G, g->d_sup, g->d_stamp, g->d_mins, g->lists);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(truss_peel, grid, block, 0, e->stream, g->d_ctl, s, G, g->d_sup, g->d_stamp, t, g->lists, (TrussPart *)g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(truss_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, (const TrussPart *)g->d_part);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const TrussRec &rc, uint64_t round_ns) {
    if (k_per_round) k_per_round[s] = rc.k;
    if (size_per_round) size_per_round[s] = (int64_t)rc.size;
    if (walked_per_round) walked_per_round[s] = (int64_t)rc.walked;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_truss: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  if (max_rounds == 0) {   // (no batch ran, so nothing was read back: the support pass alone)
    HIP_TRY(e, hipMemcpyAsync(g->h_ctl, g->d_ctl, sizeof(TrussCtl), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, ms_between(e->ev0, e->ev1, &total));
  }
  // (the control block as the last readback left it in h_ctl)
  *max_truss = g->h_ctl->max_truss;
  *levels = g->h_ctl->levels;
  *rounds = it;
  *complete = done ? 1 : 0;
  *triangles = g->h_ctl->hits / 3;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- greedy vertex colouring in Jones-Plassmann rounds (color.hip.h) ---------------------------------------------------
// The GraphHandle base serves run_batches (control block, pinned copy, events).  As in sh_core_graph the symmetric lists
// use d_in_ptr / d_in_col alone (adj_ptr / adj_col).  d_ctl: GCOL_CTL_BYTES, followed by the WlParts of gcol_assign.
// There are no piece lists: a work list keeps the vertices of the workgroup class at its far end.
struct sh_color_graph : GraphHandle<ColorCtl> {
  int64_t max_degree = 0;
  uint32_t *d_deg = nullptr;
  int32_t *d_wait = nullptr;
  ColorLists lists = {};
};
static_assert(sizeof(ColorCtl) <= GCOL_CTL_BYTES, "the control block is accounted as GCOL_CTL_BYTES (sh_color_graph_footprint)");
static_assert(sizeof(WlPart) * GCOL_MAX_BLOCKS == GCOL_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(ColorCtl::rec) / sizeof(ColorRec) == GCOL_BATCH, "one record per round of a batch");
static constexpr const char *COLOR_CREATE = "sh_color_graph_create";

extern "C" {

int sh_color_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_color_graph **out) {
  return create_graph_handle<sh_color_graph>(e, COLOR_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_color_graph *g) -> int {
    int rc;
    g->rows = rows; g->nnz = nnz;
    SymLists s;
    {
      DevArrays tmp;
      if ((rc = build_symmetric_lists(e, COLOR_CREATE, g->dev, tmp, rows, nnz, row_ptr, col_idx, val, &s)))
        return rc;
    }
    g->d_in_ptr = s.ptr; g->d_in_col = s.col; g->d_deg = s.deg;
    g->edges = s.u.M; g->max_degree = s.max_degree;
    HIP_TRY(e, g->dev.alloc(&g->d_wait, rows * 4));
    for (int i = 0; i < 2; i++)
      HIP_TRY(e, g->dev.alloc(&g->lists.list[i], rows * 4));   // a vertex joins a work list once per call (color.hip.h, invariant 1)
    return open_control(e, g, GCOL_CTL_BYTES, GCOL_CTL_BYTES + GCOL_PART_BYTES);
  });
}

int sh_color_graph_free(sh_engine *e, sh_color_graph *g) { return free_handle(e, g); }

int sh_color_graph_footprint(const sh_color_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_color_graph_edges(const sh_color_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_color_graph_max_degree(const sh_color_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_degree); }

int sh_color(sh_engine *e, sh_color_graph *g, sh_vec *color, sh_vec *prio, int32_t order, uint32_t seed, int32_t window,
             int32_t max_rounds, int32_t *colors, int32_t *rounds, int32_t *complete, int64_t *coloured,
             int64_t *size_per_round, int64_t *edges_per_round, uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (order < 0 || order > 2)
    return fail(e, SH_EINVAL, "sh_color: order = %d, must be 0 (natural), 1 (random) or 2 (largest degree first)", (int)order);
  if (window != 0 && (window < 64 || window > GCOL_WINDOW || window % 64 != 0))
    return fail(e, SH_EINVAL, "sh_color: window = %d, must be 0 or a multiple of 64 in [64, %d]", (int)window, GCOL_WINDOW);
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_color: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (!e || !g || !color || !colors || !rounds || !complete)
    return fail(e, SH_EINVAL, "sh_color: NULL argument (engine, graph, color, colors, rounds or complete)");
  const int64_t rows = g->rows;
  if (color->n < rows)
    return fail(e, SH_ESHAPE, "sh_color: color is shorter than the graph's %lld rows", (long long)rows);
  if (prio && prio->n < rows)
    return fail(e, SH_ESHAPE, "sh_color: prio is shorter than the graph's %lld rows", (long long)rows);
  *colors = 0; *rounds = 0; *complete = 1;
  if (coloured) *coloured = 0;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, GCOL_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const ColorGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col};
  const ColorOrder O{prio ? (const int32_t *)prio->d : order == 2 ? (const int32_t *)g->d_deg : nullptr, order, seed};
  const int32_t win = window == 0 ? GCOL_WINDOW : window;
  int32_t *c = (int32_t *)color->d;
  uint64_t total = 0;
  // nothing coloured; every vertex waits for the neighbours that precede it; those that wait for none make round 0
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, GCOL_CTL_BYTES, e->stream));
  uint32_t *far1 = g->lists.list[1] + (rows - 1);   // (list 1 is empty until round 0 fills it: its far end lends itself)
  hipLaunchKernelGGL(gcol_init, grid, block, 0, e->stream, g->d_ctl, G, g->d_wait, c, far1);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(gcol_count, grid, block, 0, e->stream, g->d_ctl, G, O, g->d_wait, far1);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(gcol_ready, grid, block, 0, e->stream, g->d_ctl, G, g->d_wait, g->lists);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its turn
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(gcol_assign, grid, block, 0, e->stream, g->d_ctl, s, G, win, g->d_wait, c, g->lists, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(gcol_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, (int32_t)rows, nblocks, g->d_part);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const ColorRec &rc, uint64_t round_ns) {
    if (size_per_round) size_per_round[s] = (int64_t)rc.size;
    if (edges_per_round) edges_per_round[s] = (int64_t)rc.edges;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_color: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // (the control block as the last batch's readback left it in h_ctl)
  *colors = g->h_ctl->colors;
  *rounds = it;
  *complete = done ? 1 : 0;
  if (coloured) *coloured = (int64_t)g->h_ctl->coloured;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- minimum spanning forest by Boruvka rounds on an edge list (msf.hip.h) ---------------------------------------------
// The GraphHandle base serves run_batches (control block, pinned copy, events); its list fields stay empty: the search
// walks a flat list of edge ids and needs no adjacency lists.  d_ctl: MSF_CTL_BYTES, followed by the WlParts of msf_link
// and those of the jumps.
struct sh_msf_graph : GraphHandle<MsfCtl> {
  uint32_t *d_p = nullptr, *d_to = nullptr, *d_wk = nullptr;
  uint64_t *d_best = nullptr;   // (after the last round: top, one word per vertex)
  int32_t *d_eu = nullptr, *d_ev = nullptr;
  MsfLists lists = {};
  WlPart *d_jpart = nullptr;
};
static_assert(sizeof(MsfCtl) <= MSF_CTL_BYTES, "the control block is accounted as MSF_CTL_BYTES (sh_msf_graph_footprint)");
static_assert(sizeof(WlPart) * MSF_MAX_BLOCKS == MSF_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(MsfCtl::rec) / sizeof(MsfRec) == MSF_BATCH, "one record per round of a batch");
// sh_msf_graph_footprint: p, to (4 bytes per row), best (8); eu, ev, wk and two work lists (4 bytes per edge each)
static_assert(MSF_CTL_BYTES + 2 * MSF_PART_BYTES == 33792, "the header states 16 * rows + 20 * edges + 33792");
static constexpr const char *MSF_CREATE = "sh_msf_graph_create";

// What sh_msf_graph and sh_match_graph are made of (fn: whose create this is): the edges of the simple undirected graph
// under the entries as a flat list -- eu[M] < ev[M] the ends of the e-th smallest pair, wk[M] = k(weight) of the smallest
// entry of each -- and two work lists of M edge ids, all owned by the handle; g->rows, g->nnz and g->edges are set.
// Returns with the stream synchronised: the temporaries are released.
static int build_weighted_edges(sh_engine *e, const char *fn, GraphBase *g, int64_t rows, int64_t nnz, const int32_t *row_ptr,
                                const int32_t *col_idx, const void *val, int32_t **eu, int32_t **ev, uint32_t **wk, MsfLists *lists) {
  int rc;
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  DevArrays build;   // (what build_und_edges left: the arrays as given, the sorted keys, their run heads and the scan of those)
  uint32_t *t_deg = nullptr;   // (build_und_edges counts the degrees; neither handle has a use for them)
  HIP_TRY(e, build.alloc(&t_deg, rows * 4));
  HIP_TRY(e, hipMemsetAsync(t_deg, 0, (size_t)std::max<int64_t>(rows, 1) * 4, e->stream));
  UndEdges u;
  if ((rc = build_und_edges(e, build, rows, nnz, row_ptr, col_idx, val, t_deg, &u)))
    return rc;
  const int64_t M = u.M;
  if (2 * M > 0x7FFFFF00ll)
    return fail(e, SH_EINVAL, "%s: twice the %lld edges must be at most 2^31 - 256", fn, (long long)M);
  g->edges = M;
  HIP_TRY(e, own.alloc(eu, M * 4));
  HIP_TRY(e, own.alloc(ev, M * 4));
  HIP_TRY(e, own.alloc(wk, M * 4));
  for (int i = 0; i < 2; i++)
    HIP_TRY(e, own.alloc(&lists->list[i], M * 4));   // an edge joins a work list once per round (msf.hip.h, invariant 1)
  if (M > 0) {
    const dim3 blk(WL_BS);
    const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
    hipLaunchKernelGGL(wl_edge_ends, grid_for(u.S), blk, 0, e->stream, u.sorted, u.head, u.pos, u.S, u.bits, *eu, *ev);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipMemsetAsync(*wk, 0xFF, (size_t)M * 4, e->stream));
    hipLaunchKernelGGL(msf_weights, grid_for(nnz), blk, 0, e->stream, u.rp, u.ci, u.val, nnz, (int32_t)rows, *eu, *ev, M, *wk);
    HIP_TRY(e, hipGetLastError());
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));   // (the kernels above read `build`)
  return SH_OK;
}

extern "C" {

int sh_msf_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_msf_graph **out) {
  return create_graph_handle<sh_msf_graph>(e, MSF_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_msf_graph *g) -> int {
    int rc;
    if ((rc = build_weighted_edges(e, MSF_CREATE, g, rows, nnz, row_ptr, col_idx, val, &g->d_eu, &g->d_ev, &g->d_wk, &g->lists)))
      return rc;
    DevArrays &own = g->dev;
    HIP_TRY(e, own.alloc(&g->d_p, rows * 4));
    HIP_TRY(e, own.alloc(&g->d_to, rows * 4));
    HIP_TRY(e, own.alloc(&g->d_best, rows * 8));
    if ((rc = open_control(e, g, MSF_CTL_BYTES, MSF_CTL_BYTES + 2 * MSF_PART_BYTES)))
      return rc;
    g->d_jpart = (WlPart *)((char *)g->d_ctl + MSF_CTL_BYTES + MSF_PART_BYTES);
    return SH_OK;
  });
}

int sh_msf_graph_free(sh_engine *e, sh_msf_graph *g) { return free_handle(e, g); }

int sh_msf_graph_footprint(const sh_msf_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_msf_graph_edges(const sh_msf_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_msf(sh_engine *e, sh_msf_graph *g, sh_vec *in_msf, sh_vec *comp, sh_vec *edge_u, sh_vec *edge_v, sh_vec *weight,
           int32_t max_rounds, int64_t *tree_edges, int64_t *components, int32_t *rounds, int32_t *complete,
           int64_t *walked_per_round, int64_t *kept_per_round, int64_t *hooks_per_round, int64_t *jumps_per_round,
           uint64_t *ns_per_round, uint64_t *total_ns) {
  // what the scalar alone decides comes first: no handle is needed to be told
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_msf: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (!e || !g || !in_msf || !tree_edges || !components || !rounds || !complete)
    return fail(e, SH_EINVAL, "sh_msf: NULL argument (engine, graph, in_msf, tree_edges, components, rounds or complete)");
  const int64_t rows = g->rows, M = g->edges;
  const struct { const sh_vec *v; const char *name; } vecs[] = {{in_msf, "in_msf"}, {edge_u, "edge_u"}, {edge_v, "edge_v"}, {weight, "weight"}};
  for (const auto &x : vecs)
    if (x.v && x.v->n < M)
      return fail(e, SH_ESHAPE, "sh_msf: %s is shorter than the graph's %lld edges", x.name, (long long)M);
  if (comp && comp->n < rows)
    return fail(e, SH_ESHAPE, "sh_msf: comp is shorter than the graph's %lld rows", (long long)rows);
  *tree_edges = 0; *components = 0; *rounds = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, MSF_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const MsfEdges E{(int32_t)M, g->d_eu, g->d_ev, g->d_wk};
  uint32_t *p = g->d_p;
  int32_t *chosen = (int32_t *)in_msf->d;
  uint64_t total = 0, ns = 0;
  // every vertex a tree of its own, list 0 holds every edge
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, MSF_CTL_BYTES, e->stream));
  if (edge_u && M > 0) HIP_TRY(e, hipMemcpyAsync(edge_u->d, g->d_eu, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  if (edge_v && M > 0) HIP_TRY(e, hipMemcpyAsync(edge_v->d, g->d_ev, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(msf_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, E, p, g->d_best, g->lists.list[0], chosen,
                     weight ? (uint32_t *)weight->d : nullptr);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its turn (and, behind the
  // find, unless it kept an edge; for a jumping launch after the first, unless the one before it changed a pointer)
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(msf_find, grid, block, 0, e->stream, g->d_ctl, s, E, p, g->d_best, g->lists);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(msf_pick, grid, block, 0, e->stream, g->d_ctl, s, (int32_t)rows, E, p, g->d_best, g->d_to, chosen);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(msf_link, grid, block, 0, e->stream, g->d_ctl, s, (int32_t)rows, p, g->d_best, g->d_to, g->d_part);
    HIP_TRY(e, hipGetLastError());
    for (int i = 0; i < MSF_SWEEPS; i++) {
      hipLaunchKernelGGL(msf_jump, grid, block, 0, e->stream, g->d_ctl, s, i, (int32_t)rows, p, g->d_jpart);
      HIP_TRY(e, hipGetLastError());
    }
    hipLaunchKernelGGL(msf_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part, g->d_jpart);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const MsfRec &rc, uint64_t round_ns) {
    if (walked_per_round) walked_per_round[s] = (int64_t)rc.walked;
    if (kept_per_round) kept_per_round[s] = (int64_t)rc.kept;
    if (hooks_per_round) hooks_per_round[s] = (int64_t)rc.hooks;
    if (jumps_per_round) jumps_per_round[s] = (int64_t)rc.jumps;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_msf: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // the largest index of every tree (best's memory holds nothing now), the labels (or -1 everywhere) and the roots
  uint32_t *top = (uint32_t *)g->d_best;
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  if (done) {
    HIP_TRY(e, hipMemsetAsync(top, 0, (size_t)rows * 4, e->stream));
    hipLaunchKernelGGL(msf_top, grid, block, 0, e->stream, (int32_t)rows, p, top);
    HIP_TRY(e, hipGetLastError());
  }
  hipLaunchKernelGGL(msf_label, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, done ? 1 : 0, p, top, comp ? (int32_t *)comp->d : nullptr);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  HIP_TRY(e, hipMemcpyAsync(g->h_ctl, g->d_ctl, sizeof(MsfCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  total += ns;
  *components = (int64_t)g->h_ctl->components;
  *tree_edges = rows - *components;
  *rounds = it;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- greedy weighted matching by rounds of locally dominant edges on an edge list (match.hip.h) ------------------------
// As sh_msf_graph: the GraphHandle base serves run_batches, its list fields stay empty.  d_ctl: MATCH_CTL_BYTES, followed
// by the WlParts of match_take.  mate is the caller's vector.
struct sh_match_graph : GraphHandle<MatchCtl> {
  uint32_t *d_wk = nullptr;
  uint64_t *d_best = nullptr;
  int32_t *d_eu = nullptr, *d_ev = nullptr;
  MsfLists lists = {};
};
static_assert(sizeof(MatchCtl) <= MATCH_CTL_BYTES, "the control block is accounted as MATCH_CTL_BYTES (sh_match_graph_footprint)");
static_assert(sizeof(WlPart) * MATCH_MAX_BLOCKS == MATCH_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(MatchCtl::rec) / sizeof(MatchRec) == MATCH_BATCH, "one record per round of a batch");
// sh_match_graph_footprint: best (8 bytes per row); eu, ev, wk and two work lists (4 bytes per edge each)
static_assert(MATCH_CTL_BYTES + MATCH_PART_BYTES == 17408, "the header states 8 * rows + 20 * edges + 17408");
static constexpr const char *MATCH_CREATE = "sh_match_graph_create";

extern "C" {

int sh_match_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                          const void *val, sh_match_graph **out) {
  return create_graph_handle<sh_match_graph>(e, MATCH_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_match_graph *g) -> int {
    int rc;
    if ((rc = build_weighted_edges(e, MATCH_CREATE, g, rows, nnz, row_ptr, col_idx, val, &g->d_eu, &g->d_ev, &g->d_wk, &g->lists)))
      return rc;
    HIP_TRY(e, g->dev.alloc(&g->d_best, rows * 8));
    return open_control(e, g, MATCH_CTL_BYTES, MATCH_CTL_BYTES + MATCH_PART_BYTES);
  });
}

int sh_match_graph_free(sh_engine *e, sh_match_graph *g) { return free_handle(e, g); }

int sh_match_graph_footprint(const sh_match_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_match_graph_edges(const sh_match_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_match(sh_engine *e, sh_match_graph *g, sh_vec *mate, sh_vec *in_match, sh_vec *edge_u, sh_vec *edge_v, sh_vec *weight,
             int32_t heavy, uint32_t seed, int32_t max_rounds, int64_t *pairs, int32_t *rounds, int32_t *complete,
             int64_t *walked_per_round, int64_t *kept_per_round, int64_t *matched_per_round, uint64_t *ns_per_round,
             uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (max_rounds < 1)
    return fail(e, SH_EINVAL, "sh_match: max_rounds = %d, must be at least 1", (int)max_rounds);
  if (heavy != 0 && heavy != 1)
    return fail(e, SH_EINVAL, "sh_match: heavy = %d, must be 0 (lightest first) or 1 (heaviest first)", (int)heavy);
  if (!e || !g || !mate || !pairs || !rounds || !complete)
    return fail(e, SH_EINVAL, "sh_match: NULL argument (engine, graph, mate, pairs, rounds or complete)");
  const int64_t rows = g->rows, M = g->edges;
  if (mate->n < rows)
    return fail(e, SH_ESHAPE, "sh_match: mate is shorter than the graph's %lld rows", (long long)rows);
  const struct { const sh_vec *v; const char *name; } vecs[] = {{in_match, "in_match"}, {edge_u, "edge_u"}, {edge_v, "edge_v"}, {weight, "weight"}};
  for (const auto &x : vecs)
    if (x.v && x.v->n < M)
      return fail(e, SH_ESHAPE, "sh_match: %s is shorter than the graph's %lld edges", x.name, (long long)M);
  *pairs = 0; *rounds = 0; *complete = 1;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, MATCH_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const MsfEdges E{(int32_t)M, g->d_eu, g->d_ev, g->d_wk};
  const MatchOrder O{heavy ? 0xFFFFFFFFu : 0u, seed};
  int32_t *m = (int32_t *)mate->d;
  int32_t *chosen = in_match ? (int32_t *)in_match->d : nullptr;
  uint64_t total = 0;
  int64_t found = 0;
  // every vertex free, list 0 holds every edge
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, MATCH_CTL_BYTES, e->stream));
  if (edge_u && M > 0) HIP_TRY(e, hipMemcpyAsync(edge_u->d, g->d_eu, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  if (edge_v && M > 0) HIP_TRY(e, hipMemcpyAsync(edge_v->d, g->d_ev, (size_t)M * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(match_init, grid, block, 0, e->stream, g->d_ctl, (int32_t)rows, E, m, g->d_best, g->lists.list[0], chosen,
                     weight ? (uint32_t *)weight->d : nullptr);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a round: each returns at once unless the control block says the round is its turn (and, behind the
  // bid, unless it kept an edge)
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(match_bid, grid, block, 0, e->stream, g->d_ctl, s, E, O, m, g->d_best, g->lists);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(match_take, grid, block, 0, e->stream, g->d_ctl, s, E, O, g->d_best, m, chosen, g->lists, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(match_clear, grid, block, 0, e->stream, g->d_ctl, s, E, g->d_best, g->lists);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(match_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const MatchRec &rc, uint64_t round_ns) {
    found += (int64_t)rc.matched;
    if (walked_per_round) walked_per_round[s] = (int64_t)rc.walked;
    if (kept_per_round) kept_per_round[s] = (int64_t)rc.kept;
    if (matched_per_round) matched_per_round[s] = (int64_t)rc.matched;
    if (ns_per_round) ns_per_round[s] = round_ns;
  };
  const int rc = run_batches(e, "sh_match: round", g, max_rounds, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  *pairs = found;
  *rounds = it;
  *complete = done ? 1 : 0;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- reverse Cuthill-McKee ordering in level-synchronous steps (rcm.hip.h) ----------------------------------------------
// The GraphHandle base serves run_batches.  The symmetric lists stand over the LABELS (the vertices sorted by (deg, index))
// in d_in_ptr / d_in_col; d_S maps a label back to its vertex.  d_ctl: RCM_CTL_BYTES, followed by the WlParts of a step
// and the RcmFins of the closing launch.
struct sh_rcm_graph : GraphHandle<RcmCtl> {
  int64_t max_degree = 0, zeros = 0;   // the longest list; the vertices without an edge (labels 0 .. zeros - 1)
  int32_t *d_S = nullptr;
  RcmState st = {};
  RcmFin *d_fin = nullptr;
};
static_assert(sizeof(RcmCtl) <= RCM_CTL_BYTES, "the control block is accounted as RCM_CTL_BYTES (sh_rcm_graph_footprint)");
static_assert(sizeof(WlPart) * RCM_MAX_BLOCKS == RCM_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(RcmFin) * RCM_MAX_BLOCKS == RCM_FIN_BYTES, "one RcmFin per workgroup");
static_assert(sizeof(RcmCtl::rec) / sizeof(RcmRec) == RCM_BATCH, "one record per step of a batch");
// sh_rcm_graph_footprint: ptr; S, order, posl, levl, stamp, owner and cnt (4 bytes per row each); col (8 bytes per edge)
static_assert(RCM_CTL_BYTES + RCM_PART_BYTES + RCM_FIN_BYTES == 50176, "the header states 4 * (rows + 1) + 28 * rows + 8 * edges + 50176");
static constexpr const char *RCM_CREATE = "sh_rcm_graph_create";

// The lists of an RCM handle from host CSR arrays: the edges of the simple graph and the degrees (build_und_edges), the
// vertices sorted by deg << 32 | index (S and its inverse), every edge as two keys over the labels, sorted, the list
// starts taken from them (build_symmetric_lists' second half, over labels).  Returns with the stream synchronised.
static int build_label_lists(sh_engine *e, sh_rcm_graph *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                             const void *val) {
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  DevArrays scratch;   // what the build needs while it runs
  HIP_TRY(e, own.alloc(&g->d_in_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_S, rows * 4));
  HIP_TRY(e, hipMemsetAsync(g->d_in_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  uint32_t *t_deg = nullptr, *t_inv = nullptr, *t_two = nullptr;   // t_two: the labels without an edge, the longest list
  uint64_t *t_vkey = nullptr, *t_vsorted = nullptr;
  HIP_TRY(e, scratch.alloc(&t_deg, rows * 4));
  HIP_TRY(e, scratch.alloc(&t_inv, rows * 4));
  HIP_TRY(e, scratch.alloc(&t_vkey, rows * 8));
  HIP_TRY(e, scratch.alloc(&t_vsorted, rows * 8));
  HIP_TRY(e, scratch.alloc(&t_two, 8));
  HIP_TRY(e, hipMemsetAsync(t_deg, 0, (size_t)std::max<int64_t>(rows, 1) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(t_two, 0, 8, e->stream));
  UndEdges u;
  const int rc = build_und_edges(e, scratch, rows, nnz, row_ptr, col_idx, val, t_deg, &u);
  if (rc)
    return rc;
  const int64_t S = u.S, M = u.M, E = 2 * M;
  if (E > 0x7FFFFF00ll)
    return fail(e, SH_EINVAL, "%s: the lists hold %lld entries (twice the %lld edges), must be at most 2^31 - 256", RCM_CREATE,
                (long long)E, (long long)M);
  g->edges = M;
  HIP_TRY(e, own.alloc(&g->d_in_col, E * 4));
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  if (rows > 0) {
    hipLaunchKernelGGL(rcm_vertex_keys, grid_for(rows), blk, 0, e->stream, t_deg, rows, t_vkey);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_vkey, t_vsorted, rows, 64));
    hipLaunchKernelGGL(rcm_labels, grid_for(rows), blk, 0, e->stream, t_vsorted, rows, g->d_S, t_inv, t_two);
    HIP_TRY(e, hipGetLastError());
  }
  if (M > 0) {
    uint64_t *t_key = nullptr, *t_sorted = nullptr;
    HIP_TRY(e, scratch.alloc(&t_key, E * 8));
    HIP_TRY(e, scratch.alloc(&t_sorted, E * 8));
    hipLaunchKernelGGL(rcm_both_ways, grid_for(S), blk, 0, e->stream, u.sorted, u.head, u.pos, S, u.bits, t_inv, t_key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_key, t_sorted, E, 2 * u.bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(E, rows + 1)), blk, 0, e->stream, t_sorted, E, rows, u.bits, g->d_in_ptr, g->d_in_col);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wl_max_len, dim3((unsigned)std::max(1, std::min(e->n_cus * 4, RCM_MAX_BLOCKS))), blk, 0, e->stream, g->d_in_ptr, rows,
                       t_two + 1);
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t two[2] = {0, 0};
  HIP_TRY(e, hipMemcpyAsync(two, t_two, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->zeros = (int64_t)two[0];
  g->max_degree = (int64_t)two[1];
  return SH_OK;
}

extern "C" {

int sh_rcm_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                        const void *val, sh_rcm_graph **out) {
  return create_graph_handle<sh_rcm_graph>(e, RCM_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_rcm_graph *g) -> int {
    int rc;
    if ((rc = build_label_lists(e, g, rows, nnz, row_ptr, col_idx, val)))
      return rc;
    HIP_TRY(e, g->dev.alloc(&g->st.order, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.posl, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.levl, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.stamp, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.owner, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.cnt, rows * 4));
    if ((rc = open_control(e, g, RCM_CTL_BYTES, RCM_CTL_BYTES + RCM_PART_BYTES + RCM_FIN_BYTES)))
      return rc;
    g->d_fin = (RcmFin *)((char *)g->d_ctl + RCM_CTL_BYTES + RCM_PART_BYTES);
    return SH_OK;
  });
}

int sh_rcm_graph_free(sh_engine *e, sh_rcm_graph *g) { return free_handle(e, g); }

int sh_rcm_graph_footprint(const sh_rcm_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_rcm_graph_edges(const sh_rcm_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_rcm_graph_max_degree(const sh_rcm_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_degree); }

int sh_rcm(sh_engine *e, sh_rcm_graph *g, sh_vec *perm, sh_vec *pos, sh_vec *level, int32_t sweeps, int32_t reverse, int32_t max_steps,
           int32_t *components, int32_t *sweeps_run, int32_t *steps, int32_t *complete,
           int64_t *bandwidth_before, int64_t *bandwidth_after, int64_t *profile_before, int64_t *profile_after,
           int32_t *kind_per_step, int64_t *size_per_step, int64_t *edges_per_step, uint64_t *ns_per_step, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (sweeps < 0 || sweeps > RCM_MAX_SWEEPS)
    return fail(e, SH_EINVAL, "sh_rcm: sweeps = %d, must be in [0, %d]", (int)sweeps, RCM_MAX_SWEEPS);
  if (reverse != 0 && reverse != 1)
    return fail(e, SH_EINVAL, "sh_rcm: reverse = %d, must be 0 (Cuthill-McKee) or 1 (reversed)", (int)reverse);
  if (max_steps < 1)
    return fail(e, SH_EINVAL, "sh_rcm: max_steps = %d, must be at least 1", (int)max_steps);
  if (!e || !g || !perm || !components || !sweeps_run || !steps || !complete || !bandwidth_before || !bandwidth_after ||
      !profile_before || !profile_after)
    return fail(e, SH_EINVAL, "sh_rcm: NULL argument (engine, graph, perm, components, sweeps_run, steps, complete, or a bandwidth or profile)");
  const int64_t rows = g->rows;
  const struct { const sh_vec *v; const char *name; } vecs[] = {{perm, "perm"}, {pos, "pos"}, {level, "level"}};
  for (const auto &x : vecs)
    if (x.v && x.v->n < rows)
      return fail(e, SH_ESHAPE, "sh_rcm: %s is shorter than the graph's %lld rows", x.name, (long long)rows);
  *components = 0; *sweeps_run = 0; *steps = 0; *complete = 1;
  *bandwidth_before = 0; *bandwidth_after = 0; *profile_before = 0; *profile_after = 0;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, RCM_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const RcmGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col};
  const RcmState &St = g->st;
  uint64_t total = 0;
  // the vertices without an edge take the first positions; the walk stands at the first vertex that has one
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, RCM_CTL_BYTES, e->stream));
  hipLaunchKernelGGL(rcm_init, grid, block, 0, e->stream, G, St, (uint32_t)g->zeros);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(rcm_begin, dim3(1), block, 0, e->stream, g->d_ctl, (int32_t)rows, St, (uint32_t)g->zeros, sweeps);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  int32_t it = 0;
  bool done = false;
  // the launches of a step: each returns at once unless the control block says the step is its turn and of its kind
  const auto enqueue = [&](int s, int k) {
    hipLaunchKernelGGL(rcm_sweep, grid, block, 0, e->stream, g->d_ctl, s, G, St, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(rcm_claim, grid, block, 0, e->stream, g->d_ctl, s, G, St);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(rcm_count, grid, block, 0, e->stream, g->d_ctl, s, G, St, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(rcm_place, grid, block, 0, e->stream, g->d_ctl, s, G, St, g->d_part);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(rcm_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, (int32_t)rows, nblocks, g->d_part, St);
    HIP_TRY(e, hipGetLastError());
    return (int)SH_OK;
  };
  const auto take = [&](int s, const RcmRec &rc, uint64_t step_ns) {
    if (kind_per_step) kind_per_step[s] = rc.kind;
    if (size_per_step) size_per_step[s] = (int64_t)rc.size;
    if (edges_per_step) edges_per_step[s] = (int64_t)rc.edges;
    if (ns_per_step) ns_per_step[s] = step_ns;
  };
  const int rc = run_batches(e, "sh_rcm: step", g, max_steps, &it, &done, &total, enqueue, take);
  if (rc)
    return rc;
  // the closing launch: perm, pos and level through S; bandwidth and profile before and after
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  hipLaunchKernelGGL(rcm_finish, grid, block, 0, e->stream, g->d_ctl, G, St, g->d_S, reverse, (int32_t *)perm->d,
                     pos ? (int32_t *)pos->d : nullptr, level ? (int32_t *)level->d : nullptr, g->d_fin);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(rcm_total, dim3(1), block, 0, e->stream, g->d_ctl, nblocks, g->d_fin);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  HIP_TRY(e, hipMemcpyAsync(g->h_ctl, g->d_ctl, sizeof(RcmCtl), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  uint64_t ns = 0;
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  total += ns;
  *components = g->h_ctl->components;
  *sweeps_run = g->h_ctl->sweeps_run;
  *steps = it;
  *complete = done ? 1 : 0;
  *bandwidth_before = g->h_ctl->bw[0];
  *profile_before = g->h_ctl->prof[0];
  *bandwidth_after = done ? g->h_ctl->bw[1] : -1;
  *profile_after = done ? g->h_ctl->prof[1] : -1;
  if (total_ns)
    *total_ns = total;
  return SH_OK;
}

} // extern "C"

// ---- betweenness centrality by Brandes' two sweeps, in float64 (bc.hip.h) ------------------------------------------------
// The GraphHandle base serves run_batches.  d_in_ptr / d_in_col and d_out_ptr / d_out_row hold the simple directed graph
// by target and by source, every list strictly ascending (d_in_w, d_out_w and the static row pieces stay NULL).
// d_ctl: BC_CTL_BYTES, followed by the WlParts of bc_expand.
struct sh_bc_graph : GraphHandle<BcCtl> {
  int64_t max_list = 0;   // the longest in- or out-list
  BcState st = {};
};
static_assert(sizeof(BcCtl) <= BC_CTL_BYTES, "the control block is accounted as BC_CTL_BYTES (sh_bc_graph_footprint)");
static_assert(sizeof(WlPart) * BC_MAX_BLOCKS == BC_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(BcCtl::rec) / sizeof(BcRec) == BC_BATCH, "one record per step of a batch");
// sh_bc_graph_footprint: in_ptr, out_ptr and lstart; level and order (4 bytes per row each), sigma and delta (8 each);
// in_col and out_col (4 bytes per edge each); two piece lists of edges / (BC_PIECE / 2) + 1 places of 8 bytes
static_assert(BC_CTL_BYTES + BC_PART_BYTES == 17408 && BC_PIECE / 2 == 1024 && sizeof(WlPiece) == 8,
              "the header states 12 * (rows + 1) + 24 * rows + 8 * edges + 16 * (edges / 1024 + 1) + 17408");
static constexpr const char *BC_CREATE = "sh_bc_graph_create";

// The lists of a BC handle from host CSR arrays: the entries that count and are no self-loops (wl_und_flag) become keys
// (r << bits | c), sorted; the first key of every run is an edge of the simple directed graph (sh_tri_graph_create's
// clean-up, without folding the two directions); the in-lists are read off the sorted keys, the out-lists off the
// flipped keys, sorted again.  Returns with the stream synchronised: the host arrays are done with.
static int build_directed_lists(sh_engine *e, sh_bc_graph *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                const void *val) {
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  DevArrays tmp;
  HIP_TRY(e, own.alloc(&g->d_in_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_out_ptr, (rows + 1) * 4));
  HIP_TRY(e, hipMemsetAsync(g->d_in_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_out_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  int32_t *t_rp = nullptr, *t_ci = nullptr;
  uint32_t *t_val = nullptr, *t_flag = nullptr, *t_pos = nullptr, *t_max = nullptr;
  uint64_t *t_key = nullptr, *t_sorted = nullptr, *t_okey = nullptr;
  int64_t S = 0, M = 0;
  const int bits = 32 - __builtin_clz((unsigned)std::max<int64_t>(rows - 1, 1));   // (rows <= 2^31 - 256)
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  HIP_TRY(e, tmp.alloc(&t_max, 4));
  HIP_TRY(e, hipMemsetAsync(t_max, 0, 4, e->stream));
  if (rows > 0 && nnz > 0) {
    HIP_TRY(e, tmp.alloc(&t_rp, (rows + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_ci, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_val, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_flag, (nnz + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_pos, (nnz + 1) * 4));
    HIP_TRY(e, hipMemcpyAsync(t_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wl_und_flag<BfsKeep>), grid_for(nnz + 1), blk, 0, e->stream, t_rp, t_ci, t_val, nnz, (int32_t)rows, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, nnz + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + nnz, 4, hipMemcpyDeviceToHost));
    S = (int64_t)n;
  }
  if (S > 0) {
    HIP_TRY(e, tmp.alloc(&t_key, S * 8));
    HIP_TRY(e, tmp.alloc(&t_sorted, S * 8));
    hipLaunchKernelGGL(bc_in_keys, grid_for(nnz), blk, 0, e->stream, t_rp, t_ci, t_flag, t_pos, nnz, (int32_t)rows, bits, t_key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_key, t_sorted, S, 2 * bits));
    // (t_flag and t_pos hold nnz + 1 >= S + 1 words: they serve the run heads and their scan)
    hipLaunchKernelGGL(wl_run_heads, grid_for(S + 1), blk, 0, e->stream, t_sorted, S, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, S + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + S, 4, hipMemcpyDeviceToHost));
    M = (int64_t)n;
  }
  g->edges = M;
  HIP_TRY(e, own.alloc(&g->d_in_col, M * 4));
  HIP_TRY(e, own.alloc(&g->d_out_row, M * 4));
  if (M > 0) {
    HIP_TRY(e, tmp.alloc(&t_okey, M * 8));
    // (t_key has been sorted from: its first M <= S words take the edges' keys, in order)
    hipLaunchKernelGGL(bc_out_keys, grid_for(S), blk, 0, e->stream, t_sorted, t_flag, t_pos, S, bits, t_key, t_okey);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(M, rows + 1)), blk, 0, e->stream, t_key, M, rows, bits, g->d_in_ptr, g->d_in_col);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_okey, t_sorted, M, 2 * bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(M, rows + 1)), blk, 0, e->stream, t_sorted, M, rows, bits, g->d_out_ptr, g->d_out_row);
    HIP_TRY(e, hipGetLastError());
    const dim3 mgrid((unsigned)std::max(1, std::min(e->n_cus * 4, BC_MAX_BLOCKS)));
    hipLaunchKernelGGL(wl_max_len, mgrid, blk, 0, e->stream, g->d_in_ptr, rows, t_max);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(wl_max_len, mgrid, blk, 0, e->stream, g->d_out_ptr, rows, t_max);
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t longest = 0;
  HIP_TRY(e, hipMemcpyAsync(&longest, t_max, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->max_list = (int64_t)longest;
  return SH_OK;
}

extern "C" {

int sh_bc_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                       const void *val, sh_bc_graph **out) {
  return create_graph_handle<sh_bc_graph>(e, BC_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_bc_graph *g) -> int {
    int rc;
    if ((rc = build_directed_lists(e, g, rows, nnz, row_ptr, col_idx, val)))
      return rc;
    const int64_t places = g->edges / (BC_PIECE / 2) + 1;   // see wl_push_pieces
    HIP_TRY(e, g->dev.alloc(&g->st.level, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.order, rows * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.lstart, (rows + 1) * 4));
    HIP_TRY(e, g->dev.alloc(&g->st.sigma, rows * 8));
    HIP_TRY(e, g->dev.alloc(&g->st.delta, rows * 8));
    HIP_TRY(e, g->dev.alloc(&g->st.pl[0], places * (int64_t)sizeof(WlPiece)));
    HIP_TRY(e, g->dev.alloc(&g->st.pl[1], places * (int64_t)sizeof(WlPiece)));
    return open_control(e, g, BC_CTL_BYTES, BC_CTL_BYTES + BC_PART_BYTES);
  });
}

int sh_bc_graph_free(sh_engine *e, sh_bc_graph *g) { return free_handle(e, g); }

int sh_bc_graph_footprint(const sh_bc_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_bc_graph_edges(const sh_bc_graph *g, int64_t *edges) { return HANDLE_GET(g, edges, g->edges); }

int sh_bc_graph_max_list(const sh_bc_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_list); }

int sh_bc(sh_engine *e, sh_bc_graph *g, const int32_t *sources, int32_t n_sources, sh_vec *bc, int32_t accumulate, sh_vec *sigma,
          sh_vec *level, int64_t *steps, int32_t *depth_per_source, int64_t *reached_per_source, double *sigma_max_per_source,
          int64_t *edges_per_source, uint64_t *ns_per_source, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (accumulate != 0 && accumulate != 1)
    return fail(e, SH_EINVAL, "sh_bc: accumulate = %d, must be 0 (bc starts from zero) or 1 (the scores are added to bc)", (int)accumulate);
  if (n_sources < 0)
    return fail(e, SH_EINVAL, "sh_bc: n_sources = %d, must be at least 0", (int)n_sources);
  if (!e || !g || !bc || (n_sources > 0 && !sources))
    return fail(e, SH_EINVAL, "sh_bc: NULL argument (engine, graph, bc, or sources of a call that has some)");
  const int64_t rows = g->rows;
  for (int32_t i = 0; i < n_sources; i++)
    if (sources[i] < 0 || (int64_t)sources[i] >= rows)
      return fail(e, SH_EINVAL, "sh_bc: sources[%d] = %d is outside [0, %lld)", (int)i, (int)sources[i], (long long)rows);
  if (bc->n < 2 * rows)
    return fail(e, SH_ESHAPE, "sh_bc: bc holds fewer than 2 elements for each of the graph's %lld rows", (long long)rows);
  if (sigma && sigma->n < 2 * rows)
    return fail(e, SH_ESHAPE, "sh_bc: sigma holds fewer than 2 elements for each of the graph's %lld rows", (long long)rows);
  if (level && level->n < rows)
    return fail(e, SH_ESHAPE, "sh_bc: level is shorter than the graph's %lld rows", (long long)rows);
  if (((uintptr_t)bc->d & 7u) || (sigma && ((uintptr_t)sigma->d & 7u)))
    return fail(e, SH_EINVAL, "sh_bc: bc or sigma is not aligned to 8 bytes");
  {
    const struct { const sh_vec *v; int64_t bytes; } outs[] = {{bc, rows * 8}, {sigma, rows * 8}, {level, rows * 4}};
    for (int i = 0; i < 3; i++)
      for (int j = i + 1; j < 3; j++) {
        if (!outs[i].v || !outs[j].v || rows == 0) continue;
        const char *a = (const char *)outs[i].v->d, *b = (const char *)outs[j].v->d;
        if (a < b + outs[j].bytes && b < a + outs[i].bytes)
          return fail(e, SH_EINVAL, "sh_bc: bc, sigma and level must not alias one another");
      }
  }
  if (steps) *steps = 0;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const int nblocks = std::max(1, std::min(e->n_cus * 4, BC_MAX_BLOCKS));
  const dim3 grid((unsigned)nblocks), block(WL_BS);
  const BcGraph G{(int32_t)rows, g->d_in_ptr, g->d_in_col, g->d_out_ptr, g->d_out_row};
  const BcState &St = g->st;
  if (!accumulate) HIP_TRY(e, hipMemsetAsync(bc->d, 0, (size_t)rows * 8, e->stream));
  uint64_t all = 0;
  int64_t all_steps = 0;
  for (int32_t i = 0; i < n_sources; i++) {
    uint64_t total = 0, ns = 0;
    int64_t walked = 0;
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    HIP_TRY(e, hipMemsetAsync(g->d_ctl, 0, BC_CTL_BYTES, e->stream));
    hipLaunchKernelGGL(bc_init, grid, block, 0, e->stream, g->d_ctl, G, St, sources[i]);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    // the forward sweep: the launches of a step, each of which returns at once unless the control block says it is its turn
    const auto enqueue = [&](int s, int k) {
      hipLaunchKernelGGL(bc_expand, grid, block, 0, e->stream, g->d_ctl, s, G, St, g->d_part);
      HIP_TRY(e, hipGetLastError());
      hipLaunchKernelGGL(bc_count, grid, block, 0, e->stream, g->d_ctl, s, G, St);
      HIP_TRY(e, hipGetLastError());
      hipLaunchKernelGGL(bc_close, dim3(1), block, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part, St);
      HIP_TRY(e, hipGetLastError());
      return (int)SH_OK;
    };
    const auto take = [&](int, const BcRec &rc, uint64_t) { walked += (int64_t)rc.edges; };
    int32_t it = 0;
    bool done = false;
    const int rc = run_batches(e, "sh_bc: step", g, (int32_t)std::min<int64_t>(rows, 0x7FFFFFFF), &it, &done, &total, enqueue, take);
    if (rc)
      return rc;
    if (!done)
      return fail(e, SH_EHIP, "sh_bc: the forward sweep of source %d did not end within %lld steps", (int)i, (long long)rows);
    // the backward sweep: the host knows the depth; level 0 is the source alone
    const int32_t depth = g->h_ctl->depth;
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    for (int32_t L = depth - 1; L >= 1; L--) {
      hipLaunchKernelGGL(bc_delta, grid, block, 0, e->stream, (int)L, G, St, (double *)bc->d);
      HIP_TRY(e, hipGetLastError());
    }
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
    total += ns;
    all += total;
    all_steps += it;
    if (depth_per_source) depth_per_source[i] = depth;
    if (reached_per_source) reached_per_source[i] = (int64_t)g->h_ctl->tail;
    if (sigma_max_per_source) memcpy(&sigma_max_per_source[i], &g->h_ctl->smax, 8);
    if (edges_per_source) edges_per_source[i] = walked;
    if (ns_per_source) ns_per_source[i] = total;
  }
  if (n_sources > 0) {   // the last source's values
    if (sigma) HIP_TRY(e, hipMemcpyAsync(sigma->d, St.sigma, (size_t)rows * 8, hipMemcpyDeviceToDevice, e->stream));
    if (level) HIP_TRY(e, hipMemcpyAsync(level->d, St.level, (size_t)rows * 4, hipMemcpyDeviceToDevice, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (steps) *steps = all_steps;
  if (total_ns) *total_ns = all;
  return SH_OK;
}

} // extern "C"

// ---- sparse triangular solve by level sets, in float64 (trsv.hip.h) ---------------------------------------------------------
// The GraphHandle base serves run_batches (the analysis).  d_in_ptr / d_in_col hold the lists (ascending (column,
// position as given)), d_val their values, d_diag the diagonal; d_order / d_lstart the level sets, d_level the level of
// every row; d_xw the float64 x of a float32 call.  The flipped lists, the keys and the work lists of the analysis are
// temporaries of the build.  d_ctl: TRSV_CTL_BYTES, followed by the WlParts of trsv_settle.
struct sh_trsv_graph : GraphHandle<TrsvCtl> {
  int32_t uplo = 0, unit = 0;
  int64_t levels = 0, max_list = 0, max_width = 0, zero_diag = 0, first_zero = -1;
  float *d_val = nullptr;
  double *d_diag = nullptr, *d_xw = nullptr;
  uint32_t *d_order = nullptr, *d_lstart = nullptr;
  int32_t *d_level = nullptr;
  std::vector<uint32_t> lstart;   // levels + 1 words: what the plan of a call is made from
};
static_assert(sizeof(TrsvCtl) <= TRSV_CTL_BYTES, "the control block is accounted as TRSV_CTL_BYTES (sh_trsv_graph_footprint)");
static_assert(sizeof(WlPart) * TRSV_MAX_BLOCKS == TRSV_PART_BYTES, "one WlPart per workgroup");
static_assert(sizeof(TrsvCtl::rec) / sizeof(TrsvRec) == TRSV_BATCH, "one record per round of a batch");
// sh_trsv_graph_footprint: ptr (4 bytes per row + 1); d and the float64 work vector (8 per row each), order and level (4
// each); col and val (4 bytes per entry each); lstart (4 per level + 1); the control block and its parts
static_assert(TRSV_CTL_BYTES + TRSV_PART_BYTES == 17408,
              "the header states 4 * (rows + 1) + 24 * rows + 8 * entries + 4 * (levels + 1) + 17408");
static constexpr const char *TRSV_CREATE = "sh_trsv_graph_create";

// One launch of a call's plan: a wide level (n == 0: trsv_level of level L0) or a run (trsv_run of levels L0 ... L0 + n - 1).
struct TrsvLaunch { int32_t L0, n; };
// The plan: a host function of lstart, thin and the cap alone.  A level is thin when it holds at most `thin` rows;
// consecutive thin levels form runs of at most `cap` levels; every other level is a launch of its own.
static void trsv_plan(const std::vector<uint32_t> &lstart, int64_t thin, int32_t cap, std::vector<TrsvLaunch> &plan) {
  const int64_t levels = (int64_t)lstart.size() - 1;
  for (int64_t L = 0; L < levels;) {
    if ((int64_t)(lstart[L + 1] - lstart[L]) > thin) { plan.push_back({(int32_t)L, 0}); L++; continue; }
    int64_t n = 0;
    while (L + n < levels && n < cap && (int64_t)(lstart[L + n + 1] - lstart[L + n]) <= thin) n++;
    plan.push_back({(int32_t)L, (int32_t)n});
    L += n;
  }
}

// The lists, the diagonal and the level sets of a TRSV handle from host CSR arrays.  Returns with the stream synchronised.
static int build_trsv(sh_engine *e, sh_trsv_graph *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                      const void *val) {
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  DevArrays tmp;
  int32_t *t_rp = nullptr, *t_ci = nullptr, *t_out_ptr = nullptr, *t_out_row = nullptr, *t_wait = nullptr;
  uint32_t *t_val = nullptr, *t_flag = nullptr, *t_pos = nullptr, *t_word = nullptr, *t_max = nullptr, *t_zero = nullptr;
  uint64_t *t_key = nullptr, *t_sorted = nullptr;
  int64_t S = 0;
  const int bits = 32 - __builtin_clz((unsigned)std::max<int64_t>(rows - 1, 1));   // (rows <= 2^31 - 256)
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  HIP_TRY(e, own.alloc(&g->d_in_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_diag, rows * 8));
  HIP_TRY(e, own.alloc(&g->d_xw, rows * 8));
  HIP_TRY(e, own.alloc(&g->d_order, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_level, rows * 4));
  HIP_TRY(e, hipMemsetAsync(g->d_in_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  HIP_TRY(e, tmp.alloc(&t_max, 4));
  HIP_TRY(e, tmp.alloc(&t_zero, 8));
  const uint32_t zero0[2] = {0u, 0xFFFFFFFFu};
  HIP_TRY(e, hipMemsetAsync(t_max, 0, 4, e->stream));
  HIP_TRY(e, hipMemcpyAsync(t_zero, zero0, 8, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, tmp.alloc(&t_rp, (rows + 1) * 4));
  HIP_TRY(e, tmp.alloc(&t_out_ptr, (rows + 1) * 4));
  HIP_TRY(e, hipMemcpyAsync(t_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemsetAsync(t_out_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  if (rows > 0 && nnz > 0) {
    HIP_TRY(e, tmp.alloc(&t_ci, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_val, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_flag, (nnz + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_pos, (nnz + 1) * 4));
    HIP_TRY(e, hipMemcpyAsync(t_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(trsv_flag, grid_for(nnz + 1), blk, 0, e->stream, t_rp, t_ci, nnz, (int32_t)rows, g->uplo, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, nnz + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + nnz, 4, hipMemcpyDeviceToHost));
    S = (int64_t)n;
  }
  if (rows > 0) {   // (a row without entries has d = +0.0 too)
    if (g->unit) HIP_TRY(e, hipMemsetAsync(g->d_diag, 0, (size_t)rows * 8, e->stream));
    else {
      hipLaunchKernelGGL(trsv_diag, grid_for(rows), blk, 0, e->stream, t_rp, t_ci, (const float *)t_val, (int32_t)rows, g->d_diag, t_zero);
      HIP_TRY(e, hipGetLastError());
    }
  }
  g->edges = S;
  HIP_TRY(e, own.alloc(&g->d_in_col, S * 4));
  HIP_TRY(e, own.alloc(&g->d_val, S * 4));
  HIP_TRY(e, tmp.alloc(&t_out_row, S * 4));
  if (S > 0) {
    HIP_TRY(e, tmp.alloc(&t_key, S * 8));
    HIP_TRY(e, tmp.alloc(&t_sorted, S * 8));
    HIP_TRY(e, tmp.alloc(&t_word, S * 4));
    hipLaunchKernelGGL(trsv_keys, grid_for(nnz), blk, 0, e->stream, t_rp, t_ci, t_val, t_flag, t_pos, nnz, (int32_t)rows, bits, t_key, t_word);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_pairs_u64_u32(e->stream, t_key, t_sorted, t_word, (uint32_t *)g->d_val, S, 2 * bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(S, rows + 1)), blk, 0, e->stream, t_sorted, S, rows, bits, g->d_in_ptr, g->d_in_col);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(trsv_flip, grid_for(S), blk, 0, e->stream, t_sorted, S, bits, t_key);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_key, t_sorted, S, 2 * bits));
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(S, rows + 1)), blk, 0, e->stream, t_sorted, S, rows, bits, t_out_ptr, t_out_row);
    HIP_TRY(e, hipGetLastError());
    const dim3 mgrid((unsigned)std::max(1, std::min(e->n_cus * 4, TRSV_MAX_BLOCKS)));
    hipLaunchKernelGGL(wl_max_len, mgrid, blk, 0, e->stream, g->d_in_ptr, rows, t_max);
    HIP_TRY(e, hipGetLastError());
  }
  int rc;
  if ((rc = open_control(e, g, TRSV_CTL_BYTES, TRSV_CTL_BYTES + TRSV_PART_BYTES)))
    return rc;
  // the analysis: gated rounds, one level each
  g->lstart.assign(1, 0u);
  if (rows > 0) {
    TrsvFlip F{(int32_t)rows, t_out_ptr, t_out_row, nullptr, g->d_level, {nullptr, nullptr}, {nullptr, nullptr}};
    const int64_t places = S / (TRSV_PIECE / 2) + 1;   // see wl_push_pieces
    HIP_TRY(e, tmp.alloc(&t_wait, rows * 4));
    F.wait = t_wait;
    for (int i = 0; i < 2; i++) {
      HIP_TRY(e, tmp.alloc(&F.list[i], rows * 4));
      HIP_TRY(e, tmp.alloc(&F.pieces[i], places * (int64_t)sizeof(WlPiece)));
    }
    const int nblocks = std::max(1, std::min(e->n_cus * 4, TRSV_MAX_BLOCKS));
    const dim3 grid((unsigned)nblocks);
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    hipLaunchKernelGGL(trsv_seed, grid, blk, 0, e->stream, g->d_ctl, (const int32_t *)g->d_in_ptr, F);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    const auto enqueue = [&](int s, int k) {
      hipLaunchKernelGGL(trsv_settle, grid, blk, 0, e->stream, g->d_ctl, s, F, g->d_part);
      HIP_TRY(e, hipGetLastError());
      hipLaunchKernelGGL(trsv_close, dim3(1), blk, 0, e->stream, g->d_ctl, k, s, nblocks, g->d_part);
      HIP_TRY(e, hipGetLastError());
      return (int)SH_OK;
    };
    const auto take = [&](int, const TrsvRec &r, uint64_t) {
      g->lstart.push_back(g->lstart.back() + r.size);
      g->max_width = std::max<int64_t>(g->max_width, (int64_t)r.size);
    };
    int32_t it = 0;
    bool done = false;
    uint64_t total = 0;
    if ((rc = run_batches(e, "sh_trsv_graph_create: round", g, (int32_t)std::min<int64_t>(rows, 0x7FFFFFFF), &it, &done, &total, enqueue, take)))
      return rc;
    if (!done || (int64_t)g->lstart.back() != rows)
      return fail(e, SH_EHIP, "sh_trsv_graph_create: the analysis settled %lld of %lld rows in %d rounds", (long long)g->lstart.back(),
                  (long long)rows, (int)it);
    g->levels = it;
    // order: one sort of (level << bits | row)
    const int lbits = 32 - __builtin_clz((unsigned)std::max<int64_t>(g->levels - 1, 1));
    uint64_t *t_lkey = nullptr, *t_lsorted = nullptr;
    HIP_TRY(e, tmp.alloc(&t_lkey, rows * 8));
    HIP_TRY(e, tmp.alloc(&t_lsorted, rows * 8));
    hipLaunchKernelGGL(trsv_rank_keys, grid_for(rows), blk, 0, e->stream, (const int32_t *)g->d_level, (int32_t)rows, bits, t_lkey);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_keys_u64(e->stream, t_lkey, t_lsorted, rows, bits + lbits));
    hipLaunchKernelGGL(trsv_order, grid_for(rows), blk, 0, e->stream, (const uint64_t *)t_lsorted, (int32_t)rows, bits, g->d_order);
    HIP_TRY(e, hipGetLastError());
  }
  HIP_TRY(e, own.alloc(&g->d_lstart, (g->levels + 1) * 4));
  HIP_TRY(e, hipMemcpyAsync(g->d_lstart, g->lstart.data(), (size_t)(g->levels + 1) * 4, hipMemcpyHostToDevice, e->stream));
  uint32_t longest = 0, zero[2] = {0u, 0xFFFFFFFFu};
  HIP_TRY(e, hipMemcpyAsync(&longest, t_max, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(zero, t_zero, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->max_list = (int64_t)longest;
  g->zero_diag = (int64_t)zero[0];
  g->first_zero = zero[0] ? (int64_t)zero[1] : -1;
  return SH_OK;   // (the flipped lists, the keys and the work lists go with tmp)
}

extern "C" {

int sh_trsv_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                         int32_t uplo, int32_t unit, sh_trsv_graph **out) {
  if (out) *out = nullptr;
  // what the scalars alone decide comes first
  if (uplo != 0 && uplo != 1)
    return fail(e, SH_EINVAL, "%s: uplo = %d, must be 0 (lower) or 1 (upper)", TRSV_CREATE, (int)uplo);
  if (unit != 0 && unit != 1)
    return fail(e, SH_EINVAL, "%s: unit = %d, must be 0 (the diagonal is stored) or 1 (it is one)", TRSV_CREATE, (int)unit);
  return create_graph_handle<sh_trsv_graph>(e, TRSV_CREATE, rows, nnz, row_ptr, col_idx, val, out, [&](sh_trsv_graph *g) -> int {
    g->uplo = uplo; g->unit = unit;
    return build_trsv(e, g, rows, nnz, row_ptr, col_idx, val);
  });
}

int sh_trsv_graph_free(sh_engine *e, sh_trsv_graph *g) { return free_handle(e, g); }

int sh_trsv_graph_footprint(const sh_trsv_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_trsv_graph_entries(const sh_trsv_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->edges); }

int sh_trsv_graph_levels(const sh_trsv_graph *g, int64_t *levels) { return HANDLE_GET(g, levels, g->levels); }

int sh_trsv_graph_max_list(const sh_trsv_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_list); }

int sh_trsv_graph_max_width(const sh_trsv_graph *g, int64_t *rows) { return HANDLE_GET(g, rows, g->max_width); }

int sh_trsv_graph_zero_diag(const sh_trsv_graph *g, int64_t *rows) { return HANDLE_GET(g, rows, g->zero_diag); }

int sh_trsv_graph_first_zero(const sh_trsv_graph *g, int64_t *row) { return HANDLE_GET(g, row, g->first_zero); }

int sh_trsv_graph_level(sh_engine *e, sh_trsv_graph *g, sh_vec *level) {
  if (!e || !g || !level)
    return fail(e, SH_EINVAL, "sh_trsv_graph_level: NULL argument (engine, graph or level)");
  if (level->n < g->rows)
    return fail(e, SH_ESHAPE, "sh_trsv_graph_level: level is shorter than the graph's %lld rows", (long long)g->rows);
  if (g->rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemcpyAsync(level->d, g->d_level, (size_t)g->rows * 4, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return SH_OK;
}

int sh_trsv(sh_engine *e, sh_trsv_graph *g, const sh_vec *b, sh_vec *x, int32_t f32, int32_t thin, int64_t *launches, int64_t *runs,
            int64_t *levels_in_runs, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (f32 != 0 && f32 != 1)
    return fail(e, SH_EINVAL, "sh_trsv: f32 = %d, must be 0 (b and x are float64) or 1 (float32)", (int)f32);
  if (thin > TRSV_THIN_MAX)
    return fail(e, SH_EINVAL, "sh_trsv: thin = %d, must be at most %d (negative: the default, %d)", (int)thin, TRSV_THIN_MAX, TRSV_THIN);
  if (!e || !g || !b || !x)
    return fail(e, SH_EINVAL, "sh_trsv: NULL argument (engine, graph, b or x)");
  const int64_t rows = g->rows, per = f32 ? 1 : 2;
  if (b->n < per * rows)
    return fail(e, SH_ESHAPE, "sh_trsv: b holds fewer than %d elements for each of the graph's %lld rows", (int)per, (long long)rows);
  if (x->n < per * rows)
    return fail(e, SH_ESHAPE, "sh_trsv: x holds fewer than %d elements for each of the graph's %lld rows", (int)per, (long long)rows);
  if (!f32 && (((uintptr_t)b->d & 7u) || ((uintptr_t)x->d & 7u)))
    return fail(e, SH_EINVAL, "sh_trsv: b or x is not aligned to 8 bytes");
  if (rows > 0 && b->d != x->d) {
    const char *pb = (const char *)b->d, *px = (const char *)x->d;
    const int64_t bytes = rows * 4 * per;
    if (pb < px + bytes && px < pb + bytes)
      return fail(e, SH_EINVAL, "sh_trsv: b and x overlap without being the same vector");
  }
  if (thin < 0) thin = TRSV_THIN;
  std::vector<TrsvLaunch> plan;
  trsv_plan(g->lstart, thin, TRSV_RUN, plan);
  int64_t n_runs = 0, in_runs = 0;
  for (const TrsvLaunch &l : plan) { n_runs += l.n > 0; in_runs += l.n; }
  if (launches) *launches = (int64_t)plan.size();
  if (runs) *runs = n_runs;
  if (levels_in_runs) *levels_in_runs = in_runs;
  if (total_ns) *total_ns = 0;
  if (rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  const TrsvLists T{g->d_in_ptr, g->d_in_col, g->d_val, g->d_diag, g->d_order};
  const TrsvIo Io{b->d, f32 ? g->d_xw : (double *)x->d, f32 ? (float *)x->d : nullptr, f32, g->unit};
  const dim3 block(WL_BS);
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  for (const TrsvLaunch &l : plan) {
    if (l.n > 0) {
      hipLaunchKernelGGL(trsv_run, dim3(1), block, 0, e->stream, l.L0, l.n, (const uint32_t *)g->d_lstart, T, Io);
    } else {
      const uint32_t a = g->lstart[l.L0], z = g->lstart[l.L0 + 1];
      const dim3 grid((unsigned)std::min<int64_t>(((int64_t)(z - a) + WL_BS - 1) / WL_BS, TRSV_MAX_BLOCKS));
      hipLaunchKernelGGL(trsv_level, grid, block, 0, e->stream, a, z, T, Io);
    }
    HIP_TRY(e, hipGetLastError());
  }
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  uint64_t ns = 0;
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  if (total_ns) *total_ns = ns;
  return SH_OK;
}

} // extern "C"

// ---- incomplete LU factorisation without fill by level sets, in float64 (ilu0.hip.h) ----------------------------------------
// d_ptr / d_col: the slots of every row in ascending column; d_dslot / d_up / d_rwork per row; d_gstart / d_perm: the
// entries of every slot in the order given; d_slot_of / d_head per input position; d_w: the float64 working array of a
// call; d_order / d_lstart the level sets and d_level the level of every row, as sh_trsv's analysis of the lower
// triangle left them; d_fig: the figures a kernel counts.  The keys and scans of the build are temporaries.
struct sh_ilu0_graph : GraphBase {
  int64_t levels = 0, max_list = 0, max_width = 0, missing_diag = 0, first_missing = -1, work = 0;
  int32_t *d_ptr = nullptr, *d_col = nullptr, *d_dslot = nullptr, *d_up = nullptr, *d_rwork = nullptr, *d_level = nullptr;
  int32_t *d_slot_of = nullptr, *d_gstart = nullptr;
  uint32_t *d_head = nullptr, *d_perm = nullptr, *d_order = nullptr, *d_lstart = nullptr, *d_fig = nullptr;
  double *d_w = nullptr;
  std::vector<uint32_t> lstart;   // levels + 1 words: what the plan of a call is made from
};
// sh_ilu0_graph_footprint: ptr (4 bytes per row + 1); dslot, up, rwork, order and level (4 per row each); slot_of, head
// and perm (4 per entry as given each); col and gstart (4 per slot, gstart one more) and w (8 per slot); lstart (4 per
// level + 1); the figures
static_assert(ILU0_FIG_BYTES == 16, "the header states 4 * (rows + 1) + 20 * rows + 12 * nnz + 16 * entries + 4 * (levels + 1) + 20");
static_assert(ILU0_THIN == TRSV_THIN && ILU0_THIN_MAX == TRSV_THIN_MAX, "thin has sh_trsv's meaning and range");
static constexpr const char *ILU0_CREATE = "sh_ilu0_graph_create";

// The slots and the level sets of an ILU(0) handle from the host CSR pattern.  Returns with the stream synchronised.
static int build_ilu0(sh_engine *e, sh_ilu0_graph *g, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx) {
  g->rows = rows; g->nnz = nnz;
  DevArrays &own = g->dev;
  HIP_TRY(e, own.alloc(&g->d_level, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_order, rows * 4));
  {   // the level sets: sh_trsv's analysis of the lower triangle, unit diagonal (it reads no value: the columns stand in)
    sh_trsv_graph t;
    t.uplo = 0; t.unit = 1;
    RC_TRY(build_trsv(e, &t, rows, nnz, row_ptr, col_idx, col_idx));
    g->levels = t.levels; g->max_width = t.max_width;
    g->lstart = t.lstart;
    if (rows > 0) {
      HIP_TRY(e, hipMemcpyAsync(g->d_level, t.d_level, (size_t)rows * 4, hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(e, hipMemcpyAsync(g->d_order, t.d_order, (size_t)rows * 4, hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
  }   // (its lists, diagonal and control block go here)
  DevArrays tmp;
  int32_t *t_rp = nullptr, *t_ci = nullptr;
  uint32_t *t_flag = nullptr, *t_pos = nullptr, *t_word = nullptr, *t_max = nullptr;
  uint64_t *t_key = nullptr, *t_sorted = nullptr;
  int64_t S = 0, E = 0;
  const int bits = 32 - __builtin_clz((unsigned)std::max<int64_t>(rows - 1, 1));   // (rows <= 2^31 - 256)
  const dim3 blk(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  HIP_TRY(e, own.alloc(&g->d_ptr, (rows + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_dslot, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_up, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_rwork, rows * 4));
  HIP_TRY(e, own.alloc(&g->d_slot_of, nnz * 4));
  HIP_TRY(e, own.alloc(&g->d_head, nnz * 4));
  HIP_TRY(e, own.alloc(&g->d_perm, nnz * 4));
  HIP_TRY(e, own.alloc(&g->d_lstart, (g->levels + 1) * 4));
  HIP_TRY(e, own.alloc(&g->d_fig, ILU0_FIG_BYTES));
  HIP_TRY(e, hipMemcpyAsync(g->d_lstart, g->lstart.data(), (size_t)(g->levels + 1) * 4, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_ptr, 0, (size_t)(rows + 1) * 4, e->stream));
  const uint32_t fig0[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
  HIP_TRY(e, hipMemcpyAsync(g->d_fig, fig0, ILU0_FIG_BYTES, hipMemcpyHostToDevice, e->stream));
  HIP_TRY(e, tmp.alloc(&t_max, 4));
  HIP_TRY(e, hipMemsetAsync(t_max, 0, 4, e->stream));
  if (rows > 0 && nnz > 0) {
    HIP_TRY(e, tmp.alloc(&t_rp, (rows + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_ci, nnz * 4));
    HIP_TRY(e, tmp.alloc(&t_flag, (nnz + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_pos, (nnz + 1) * 4));
    HIP_TRY(e, hipMemcpyAsync(t_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemcpyAsync(t_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipMemsetAsync(g->d_slot_of, 0xFF, (size_t)nnz * 4, e->stream));
    HIP_TRY(e, hipMemsetAsync(g->d_head, 0, (size_t)nnz * 4, e->stream));
    hipLaunchKernelGGL(ilu0_flag, grid_for(nnz + 1), blk, 0, e->stream, t_ci, nnz, (int32_t)rows, t_flag);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_flag, t_pos, nnz + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_pos + nnz, 4, hipMemcpyDeviceToHost));
    S = (int64_t)n;
  }
  if (S > 0) {   // key, one stable sort, heads, slots
    uint32_t *t_head = nullptr, *t_hpos = nullptr;
    HIP_TRY(e, tmp.alloc(&t_key, S * 8));
    HIP_TRY(e, tmp.alloc(&t_sorted, S * 8));
    HIP_TRY(e, tmp.alloc(&t_word, S * 4));
    HIP_TRY(e, tmp.alloc(&t_head, (S + 1) * 4));
    HIP_TRY(e, tmp.alloc(&t_hpos, (S + 1) * 4));
    hipLaunchKernelGGL(ilu0_keys, grid_for(nnz), blk, 0, e->stream, t_rp, t_ci, t_flag, t_pos, nnz, (int32_t)rows, bits, t_key, t_word);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_sort_pairs_u64_u32(e->stream, t_key, t_sorted, t_word, g->d_perm, S, 2 * bits));
    hipLaunchKernelGGL(wl_run_heads, grid_for(S + 1), blk, 0, e->stream, t_sorted, S, t_head);
    HIP_TRY(e, hipGetLastError());
    HIP_TRY(e, device_exclusive_sum_u32(e->stream, t_head, t_hpos, S + 1));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpy(&n, t_hpos + S, 4, hipMemcpyDeviceToHost));
    E = (int64_t)n;
    HIP_TRY(e, own.alloc(&g->d_col, E * 4));
    HIP_TRY(e, own.alloc(&g->d_gstart, (E + 1) * 4));
    HIP_TRY(e, own.alloc(&g->d_w, E * 8));
    hipLaunchKernelGGL(ilu0_slots, grid_for(S + 1), blk, 0, e->stream, (const uint64_t *)t_sorted, (const uint32_t *)t_head,
                       (const uint32_t *)t_hpos, (const uint32_t *)g->d_perm, S, g->d_slot_of, g->d_head, t_key, g->d_gstart);
    HIP_TRY(e, hipGetLastError());   // (t_key holds the slots' keys from here on)
    hipLaunchKernelGGL(wl_forward_lists, grid_for(std::max(E, rows + 1)), blk, 0, e->stream, t_key, E, rows, bits, g->d_ptr, g->d_col);
    HIP_TRY(e, hipGetLastError());
    const dim3 mgrid((unsigned)std::max(1, std::min(e->n_cus * 4, ILU0_MAX_BLOCKS)));
    hipLaunchKernelGGL(wl_max_len, mgrid, blk, 0, e->stream, g->d_ptr, rows, t_max);
    HIP_TRY(e, hipGetLastError());
  } else {
    HIP_TRY(e, own.alloc(&g->d_col, 0));
    HIP_TRY(e, own.alloc(&g->d_gstart, 4));
    HIP_TRY(e, own.alloc(&g->d_w, 0));
    HIP_TRY(e, hipMemsetAsync(g->d_gstart, 0, 4, e->stream));
  }
  g->edges = E;
  if (rows > 0) {
    hipLaunchKernelGGL(ilu0_diag, grid_for(rows), blk, 0, e->stream, (const int32_t *)g->d_ptr, (const int32_t *)g->d_col, (int32_t)rows,
                       g->d_dslot, g->d_up, g->d_fig);
    HIP_TRY(e, hipGetLastError());
    hipLaunchKernelGGL(ilu0_work, grid_for(rows), blk, 0, e->stream, (const int32_t *)g->d_ptr, (const int32_t *)g->d_col,
                       (const int32_t *)g->d_up, (int32_t)rows, g->d_rwork, (unsigned long long *)(g->d_fig + 2));
    HIP_TRY(e, hipGetLastError());
  }
  uint32_t longest = 0, fig[4] = {0u, 0u, 0u, 0u};
  HIP_TRY(e, hipMemcpyAsync(&longest, t_max, 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(fig, g->d_fig, ILU0_FIG_BYTES, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  g->max_list = (int64_t)longest;
  g->missing_diag = (int64_t)fig[0];
  g->first_missing = fig[0] ? (int64_t)fig[1] : -1;
  g->work = (int64_t)(((uint64_t)fig[3] << 32) | (uint64_t)fig[2]);
  return SH_OK;   // (the keys and the scans go with tmp)
}

extern "C" {

int sh_ilu0_graph_create(sh_engine *e, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, sh_ilu0_graph **out) {
  // (the pattern alone: check_host_csr's `val` is what a matrix with entries must bring, and here that is its columns)
  return create_graph_handle<sh_ilu0_graph>(e, ILU0_CREATE, rows, nnz, row_ptr, col_idx, col_idx, out,
                                            [&](sh_ilu0_graph *g) -> int { return build_ilu0(e, g, rows, nnz, row_ptr, col_idx); });
}

int sh_ilu0_graph_free(sh_engine *e, sh_ilu0_graph *g) { return free_handle(e, g); }

int sh_ilu0_graph_footprint(const sh_ilu0_graph *g, uint64_t *device_bytes) { return HANDLE_GET(g, device_bytes, (uint64_t)g->dev.bytes); }

int sh_ilu0_graph_entries(const sh_ilu0_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->edges); }

int sh_ilu0_graph_levels(const sh_ilu0_graph *g, int64_t *levels) { return HANDLE_GET(g, levels, g->levels); }

int sh_ilu0_graph_max_list(const sh_ilu0_graph *g, int64_t *entries) { return HANDLE_GET(g, entries, g->max_list); }

int sh_ilu0_graph_max_width(const sh_ilu0_graph *g, int64_t *rows) { return HANDLE_GET(g, rows, g->max_width); }

int sh_ilu0_graph_missing_diag(const sh_ilu0_graph *g, int64_t *rows) { return HANDLE_GET(g, rows, g->missing_diag); }

int sh_ilu0_graph_first_missing(const sh_ilu0_graph *g, int64_t *row) { return HANDLE_GET(g, row, g->first_missing); }

int sh_ilu0_graph_work(const sh_ilu0_graph *g, int64_t *lookups) { return HANDLE_GET(g, lookups, g->work); }

int sh_ilu0_graph_level(sh_engine *e, sh_ilu0_graph *g, sh_vec *level) {
  if (!e || !g || !level)
    return fail(e, SH_EINVAL, "sh_ilu0_graph_level: NULL argument (engine, graph or level)");
  if (level->n < g->rows)
    return fail(e, SH_ESHAPE, "sh_ilu0_graph_level: level is shorter than the graph's %lld rows", (long long)g->rows);
  if (g->rows == 0)
    return SH_OK;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipMemcpyAsync(level->d, g->d_level, (size_t)g->rows * 4, hipMemcpyDeviceToDevice, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  return SH_OK;
}

int sh_ilu0(sh_engine *e, sh_ilu0_graph *g, sh_vec *val, sh_vec *lu, int32_t f32, int32_t thin, int64_t *launches, int64_t *runs,
            int64_t *levels_in_runs, int64_t *zero_pivots, int64_t *first_zero, uint64_t *total_ns) {
  // what the scalars alone decide comes first: no handle is needed to be told
  if (f32 != 0 && f32 != 1)
    return fail(e, SH_EINVAL, "sh_ilu0: f32 = %d, must be 0 (lu is float64) or 1 (float32)", (int)f32);
  if (thin > ILU0_THIN_MAX)
    return fail(e, SH_EINVAL, "sh_ilu0: thin = %d, must be at most %d (negative: the default, %d)", (int)thin, ILU0_THIN_MAX, ILU0_THIN);
  if (!e || !g || !val || !lu)
    return fail(e, SH_EINVAL, "sh_ilu0: NULL argument (engine, graph, val or lu)");
  const int64_t rows = g->rows, nnz = g->nnz, per = f32 ? 1 : 2;
  if (val->n < nnz)
    return fail(e, SH_ESHAPE, "sh_ilu0: val holds fewer elements than the graph's %lld entries", (long long)nnz);
  if (lu->n < per * nnz)
    return fail(e, SH_ESHAPE, "sh_ilu0: lu holds fewer than %d elements for each of the graph's %lld entries", (int)per, (long long)nnz);
  if (!f32 && ((uintptr_t)lu->d & 7u))
    return fail(e, SH_EINVAL, "sh_ilu0: lu is not aligned to 8 bytes");
  if (nnz > 0 && (val->d != lu->d || !f32)) {
    const char *pv = (const char *)val->d, *pl = (const char *)lu->d;
    if (pv < pl + nnz * 4 * per && pl < pv + nnz * 4)
      return fail(e, SH_EINVAL, "sh_ilu0: val and lu overlap without being the same float32 vector");
  }
  if (thin < 0) thin = ILU0_THIN;
  std::vector<TrsvLaunch> plan;
  trsv_plan(g->lstart, thin, ILU0_RUN, plan);
  const bool any = rows > 0 && nnz > 0;   // (without entries every lu is nothing and every pivot +0.0: the host says so)
  if (!any) plan.clear();
  int64_t n_runs = 0, in_runs = 0;
  for (const TrsvLaunch &l : plan) { n_runs += l.n > 0; in_runs += l.n; }
  if (launches) *launches = any ? (int64_t)plan.size() + (g->edges > 0) + 1 : 0;   // (ilu0_load, the plan, ilu0_store)
  if (runs) *runs = n_runs;
  if (levels_in_runs) *levels_in_runs = in_runs;
  if (total_ns) *total_ns = 0;
  if (!any) {
    if (zero_pivots) *zero_pivots = rows;
    if (first_zero) *first_zero = rows > 0 ? 0 : -1;
    return SH_OK;
  }
  HIP_TRY(e, hipSetDevice(e->device));
  const Ilu0Lists T{g->d_ptr, g->d_col, g->d_dslot, g->d_up, g->d_rwork, g->d_order, g->d_w};
  const dim3 block(WL_BS);
  const auto grid_for = [](int64_t n) { return dim3((unsigned)((n + WL_BS - 1) / WL_BS)); };
  HIP_TRY(e, hipMemsetAsync(g->d_fig, 0, 4, e->stream));
  HIP_TRY(e, hipMemsetAsync(g->d_fig + 1, 0xFF, 4, e->stream));
  HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
  if (g->edges > 0) {
    hipLaunchKernelGGL(ilu0_load, grid_for(g->edges), block, 0, e->stream, (const int32_t *)g->d_gstart, (const uint32_t *)g->d_perm,
                       (const float *)val->d, g->edges, g->d_w);
    HIP_TRY(e, hipGetLastError());
  }
  for (const TrsvLaunch &l : plan) {
    if (l.n > 0) {
      hipLaunchKernelGGL(ilu0_run, dim3(1), block, 0, e->stream, l.L0, l.n, (const uint32_t *)g->d_lstart, T);
    } else {
      const uint32_t a = g->lstart[l.L0], z = g->lstart[l.L0 + 1];
      const dim3 grid((unsigned)std::min<int64_t>(((int64_t)(z - a) + WL_BS - 1) / WL_BS, ILU0_MAX_BLOCKS));
      hipLaunchKernelGGL(ilu0_level, grid, block, 0, e->stream, a, z, T);
    }
    HIP_TRY(e, hipGetLastError());
  }
  hipLaunchKernelGGL(ilu0_store, grid_for(std::max(nnz, rows)), block, 0, e->stream, (const int32_t *)g->d_slot_of,
                     (const uint32_t *)g->d_head, (const int32_t *)g->d_dslot, (const double *)g->d_w, nnz, (int32_t)rows, f32, lu->d, g->d_fig);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
  uint32_t fig[2] = {0u, 0u};
  HIP_TRY(e, hipMemcpyAsync(fig, g->d_fig, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  uint64_t ns = 0;
  HIP_TRY(e, ms_between(e->ev0, e->ev1, &ns));
  if (total_ns) *total_ns = ns;
  if (zero_pivots) *zero_pivots = (int64_t)fig[0];
  if (first_zero) *first_zero = fig[0] ? (int64_t)fig[1] : -1;
  return SH_OK;
}

} // extern "C"

#ifdef SH_PLAN_EMULATE
#include "debug_graph_tools.h"   // (behind the graph handles it fills)
#endif
