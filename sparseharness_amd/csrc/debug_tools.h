// debug_tools.h -- included by engine.hip under -DSH_PLAN_EMULATE only (the tools build, sparseharness_amd/variants/
// emulate.so; never the product build): the host emulator of the tiled / bit plans, the host-vs-device builder
// comparison, the builders' verdicts, the switches that lower the limit on P or fail a device build step, and the placement
// probes (sh_debug_*), used by tests/test_plan_cpu.py, tests/test_plan_limits_*.py, tests/test_builder_gpu.py and tools/.
// The poison hook of the graph handles, sh_debug_poison_graph, is the tools build's too but lives in debug_graph_tools.h:
// it has to stand behind the handle structs of engine.hip, which are defined after this file is included.
#pragma once
// Tools / CPU tests only (never in the product build): build the tiled plan on the host and execute BOTH phases
// on the host, entry by entry, through exactly the tables the kernels read (fold flags, obase, gdest, gblk / ptab,
// pslot, lrp) with the kernels' indexing.  A test that compares the result with a plain CSR product thereby
// checks the layout without a GPU.  semiring: 0 = (+,x) float, 2 = (or,and) int32, 3 = (max,min) int32.  stats[0..7]: stream entries,
// light entries, products, bins, chunks, heavy rows, P words never written but read (must be 0), tiles.
namespace {
struct HPlusTimes { using T = float; static T identity() { return 0.0f; } static T mul(T x, T a) { return x * a; } static T add(T a, T b) { return a + b; } };
struct HOrAnd { using T = int32_t; static T identity() { return 0; } static T mul(T x, T a) { return (x != 0) && (a != 0); } static T add(T a, T b) { return (a != 0) || (b != 0); } };
struct HMaxMin { using T = int32_t; static T identity() { return INT32_MIN; } static T mul(T x, T a) { return x < a ? x : a; } static T add(T a, T b) { return a > b ? a : b; } };
template <class T> T hbits(uint32_t u) { T v; memcpy(&v, &u, 4); return v; }
template <class T> uint32_t tobits(T v) { uint32_t u; memcpy(&u, &v, 4); return u; }

template <class SR>
int emulate(const TiledHost &H, int64_t rows, int64_t cols, const uint32_t *x, uint32_t *y, int64_t *stats) {
  using T = typename SR::T;
  constexpr uint32_t POISON = 0x7FC0DEADu;
  std::vector<uint32_t> P((size_t)H.p_len + 4, POISON), partial((size_t)H.n_partials + 1, POISON), xs((size_t)H.tcols + 4);
  const bool coded = !H.vdict.empty();
  auto value_at = [&](int64_t q) -> uint32_t {
    if (!coded) return H.tval[(size_t)q];
    if (H.code_bits == 4) return H.vdict[(H.tcode[(size_t)q >> 1] >> ((q & 1) * 4)) & 0xFu];
    if (H.code_bits == 16) return H.vdict[reinterpret_cast<const uint16_t *>(H.tcode.data())[(size_t)q]];
    return H.vdict[H.tcode[(size_t)q]];
  };
  // ---- phase 1
  for (const TileChunk &ch : H.chunks) {
    if (ch.s >= ch.e) continue;
    const int64_t c0 = (int64_t)ch.tile * H.tcols;
    for (int i = 0; i < H.tcols; i++) xs[(size_t)i] = (c0 + i < cols) ? x[c0 + i] : tobits<T>(SR::identity());
    xs[(size_t)H.tcols] = tobits<T>(SR::identity());
    const uint32_t first_mask = tcol_first_mask(H.tcols);
    auto prod = [&](int64_t q, uint32_t colmask) { return SR::mul(hbits<T>(xs[H.tcol[(size_t)q] & colmask]), hbits<T>(value_at(q))); };
    if (ch.hs > ch.s) {   // light chunk: blocks of 64 groups; a group stores 4 products unless it folds into the one in front
      if (ch.s % 256 || ch.e % 4) return -10;
      const int64_t gs = ch.s / 4, le = ch.e / 4;
      // the fold flag of group g: bit 15 of its first column code, or (wide layouts) its bit in the mask word of its block
      const bool wide = H.tcols != TCOLS;
      if (wide && H.fmask.size() != H.obase.size()) return -14;
      auto flagged = [&](int64_t g) {
        if (g >= le) return false;
        if (!wide) return (H.tcol[(size_t)g * 4] & TCOL_FOLD) != 0;
        return ((H.fmask[(size_t)ch.ob0 + (size_t)((g - gs) / 64)] >> ((g - gs) % 64)) & 1ull) != 0;
      };
      for (int64_t blk = 0; gs + blk * 64 < le; blk++) {
        int64_t pos = H.obase[(size_t)ch.ob0 + (size_t)blk];
        for (int64_t g = gs + blk * 64; g < std::min(le, gs + blk * 64 + 64); g++) {
          const int64_t lane = g - (gs + blk * 64);
          if (flagged(g)) {
            if (!(lane & 1)) return -12;   // a B group sits on an odd lane, right behind its A
            continue;
          }
          const bool takes = (lane & 1) == 0 && lane + 1 < 64 && flagged(g + 1);
          if (pos + 4 > H.p_len) return -11;
          for (int k = 0; k < 4; k++) {
            T acc = prod(g * 4 + k, k == 0 ? first_mask : 0xFFFFu);
            if (takes) acc = SR::add(acc, prod((g + 1) * 4 + k, k == 0 ? first_mask : 0xFFFFu));
            P[(size_t)pos + k] = tobits<T>(acc);
          }
          pos += 4;
        }
      }
    } else {              // heavy chunk: strips of 16, segmented scan inside waves of 64 strips
      const int64_t s0 = ch.s / HSTRIP, s1 = ch.e / HSTRIP, sbase = ch.pdelta / HSTRIP;
      for (int64_t w0 = s0; w0 < s1; w0 += 64) {
        T lane[64];
        uint32_t d[64];
        const int n = (int)std::min<int64_t>(64, s1 - w0);
        for (int l = 0; l < n; l++) {
          T t = SR::identity();
          for (int i = 0; i < HSTRIP; i++) t = SR::add(t, prod((w0 + l) * HSTRIP + i, 0xFFFFu));
          lane[l] = t;
          d[l] = H.gdest[(size_t)(w0 + l - sbase)];
        }
        for (int l = 0; l < n; l++) {
          if (!(d[l] & GD_LAST)) continue;
          const int dist = (int)((d[l] >> GD_DIST_SHIFT) & 63u);
          if (dist > l) return -13;
          T t = lane[l - dist];
          for (int k = l - dist + 1; k <= l; k++) t = SR::add(t, lane[k]);
          partial[d[l] & GD_SLOT_MASK] = tobits<T>(t);
        }
      }
    }
  }
  // ---- phase 2
  int64_t poison_reads = 0;
  std::vector<uint32_t> img((size_t)TBIN);
  for (const RowBin &b : H.bins) {
    std::fill(img.begin(), img.end(), POISON);
    const int64_t n4 = b.n / 4;
    for (int64_t k = 0; k < n4; k++) {
      const uint32_t *rec = &H.gblk[((size_t)b.gb0 + (size_t)(k / 64)) * 4];
      const int lane = (int)(k % 64);
      uint32_t below = 0;
      for (int l = 0; l < lane; l++) below += (rec[l / 32] >> (l % 32)) & 1u;
      const uint32_t own = (rec[lane / 32] >> (lane % 32)) & 1u;
      const int64_t pg = (int64_t)H.ptab[(size_t)b.pt0 + (size_t)std::max<int64_t>((int64_t)(rec[2] + below + own) - 1, 0)] + k;
      if (pg < 0 || pg * 4 + 3 >= (int64_t)P.size()) return -20;
      for (int i = 0; i < 4; i++) {
        const uint16_t sl = H.pslot[(size_t)b.pstart + (size_t)(k * 4 + i)];
        if (sl == TSLOT_PAD) continue;
        if (sl >= TBIN) return -21;
        if (img[sl] != POISON) return -22;   // two products in one slot
        img[sl] = P[(size_t)(pg * 4 + i)];
        if (img[sl] == POISON) poison_reads++;
      }
    }
    for (int64_t r = b.r0; r < (int64_t)b.r0 + b.nr; r++) {
      if (H.lrp[(size_t)r] & 0x80000000u) continue;
      const int64_t s = (int64_t)(H.lrp[(size_t)r] & 0x7FFFFFFFu) - b.csr0, e = (int64_t)(H.lrp[(size_t)r + 1] & 0x7FFFFFFFu) - b.csr0;
      if (s < 0 || e > TBIN) return -23;
      T acc = SR::identity();
      for (int64_t j = s; j < e; j++) {
        if (img[(size_t)j] == POISON) poison_reads++;
        acc = SR::add(acc, hbits<T>(img[(size_t)j]));
      }
      y[r] = tobits<T>(acc);
    }
  }
  for (const LongRow &lr : H.heavy) {
    T acc = SR::identity();
    for (int k = 0; k < lr.nslots; k++) {
      if (partial[(size_t)lr.slot0 + k] == POISON) poison_reads++;
      acc = SR::add(acc, hbits<T>(partial[(size_t)lr.slot0 + k]));
    }
    y[lr.row] = tobits<T>(acc);
  }
  if (stats) {
    stats[0] = H.stream_len; stats[1] = H.light_entries; stats[2] = H.p_len; stats[3] = (int64_t)H.bins.size();
    stats[4] = (int64_t)H.chunks.size(); stats[5] = (int64_t)H.heavy.size(); stats[6] = poison_reads;
    stats[7] = (cols + H.tcols - 1) / H.tcols;
  }
  (void)rows;
  return 0;
}
} // namespace

// The (or,and) bit plan walked on the host: y[r] = OR over the live entries of row r of (x[col] != 0), through the
// entry stream, the sub-range offsets and the item lists exactly as bits_blocks / bits_finish index them.
extern "C" int sh_debug_emulate_bits(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                     const void *val, const void *x, int32_t *y, int64_t *stats) {
  sh_plan_options opt;
  sh_plan_options_default(&opt);
  BitsHost H;
  if (!build_bits_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, H)) return -1;
  const uint32_t *xv = (const uint32_t *)x;
  std::vector<uint32_t> xbits((size_t)H.n_ct * (BITS_BC / 32), 0u), partial((size_t)std::max<size_t>(H.items.size(), 1) * (BITS_BR / 32), 0u);
  for (int64_t c = 0; c < cols; c++) if (xv[c] != 0u) xbits[(size_t)c >> 5] |= 1u << (c & 31);
  for (size_t k = 0; k < H.items.size(); k++) {
    const BitsItem &it = H.items[k];
    if ((it.s & 7) || (it.e & 7)) return -30;
    const uint32_t *xs = &xbits[(size_t)it.ct * (BITS_BC / 32)];
    uint32_t *os = &partial[k * (BITS_BR / 32)];
    for (int sub = it.sub0; sub < it.sub1; sub++) {
      const int32_t s = H.bsub[(size_t)it.soff + (sub - it.sub0)], e = H.bsub[(size_t)it.soff + (sub - it.sub0) + 1];
      if ((s & 7) || (e & 7) || s < it.s || e > it.e) return -31;
      for (int32_t q = s; q < e; q++) {
        const uint32_t w = H.ent[(size_t)q], c = w & BITS_COL_MASK;
        if ((xs[c >> 5] >> (c & 31)) & 1u) {
          const uint32_t r = (uint32_t)sub * BITS_SUB + (w >> 19);
          os[r >> 5] |= 1u << (r & 31);
        }
      }
    }
  }
  for (int64_t r = 0; r < rows; r++) {
    const int rr = (int)(r / BITS_BR);
    const uint32_t rl = (uint32_t)(r % BITS_BR);
    uint32_t w = 0;
    for (int it = H.rr_item0[(size_t)rr]; it < H.rr_item0[(size_t)rr + 1]; it++) w |= partial[(size_t)it * (BITS_BR / 32) + (rl >> 5)];
    y[r] = (int32_t)((w >> (rl & 31)) & 1u);
  }
  if (stats) { stats[0] = (int64_t)H.ent.size(); stats[1] = H.entries; stats[2] = (int64_t)H.items.size(); stats[3] = H.n_rr; stats[4] = H.n_ct; }
  return 0;
}

extern "C" int sh_debug_emulate_plan(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                     const void *val, const sh_plan_options *opt_p, int semiring, const void *x, void *y, int64_t *stats) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  TiledHost H;
  if (!build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, 256, H)) return -1;
  if (semiring == 0) return emulate<HPlusTimes>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
  if (semiring == 2) return emulate<HOrAnd>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
  if (semiring == 3) return emulate<HMaxMin>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
  return -2;
}
// sh_debug_emulate_plan for a device with n_cus CUs, and the phase-1 work items the host builder cut for it: items gets
// up to cap_items of them in launch order, 8 words each (TileChunk: tile, s, e, hs, pdelta, ob0, 0, 0; fillers have
// s == e).  x and y may both be NULL: the plan is then only built.  Returns the number of items, or the emulator's
// negative code (-1: the builder refused, -2: no such semiring).
extern "C" int64_t sh_debug_plan_items(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                       const void *val, const sh_plan_options *opt_p, int n_cus, int semiring, const void *x, void *y,
                                       int64_t *stats, int32_t *items, int64_t cap_items) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  TiledHost H;
  if (!build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, n_cus, H)) return -1;
  static_assert(sizeof(TileChunk) == 32, "8 words per work item");
  if (items) memcpy(items, H.chunks.data(), (size_t)std::min<int64_t>(cap_items, (int64_t)H.chunks.size()) * sizeof(TileChunk));
  if (x && y) {
    int rc = -2;
    if (semiring == 0) rc = emulate<HPlusTimes>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
    if (semiring == 2) rc = emulate<HOrAnd>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
    if (semiring == 3) rc = emulate<HMaxMin>(H, rows, cols, (const uint32_t *)x, (uint32_t *)y, stats);
    if (rc != 0) return rc;
  }
  return (int64_t)H.chunks.size();
}
// How the host builder codes the values of a matrix (CPU tests: which phase-1 instantiation a value set selects):
// *code_bits = 0 raw words, else 4 / 8 / 16; *distinct = the dictionary's words in use.  0, or -1: the builder refused.
extern "C" int sh_debug_plan_coding(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                    const sh_plan_options *opt_p, int32_t *code_bits, int32_t *distinct) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  TiledHost H;
  if (!build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, 256, H)) return -1;
  *code_bits = H.vdict.empty() ? 0 : H.code_bits;
  *distinct = H.vdict.empty() ? 0 : H.vdict_used;
  return 0;
}
// The layout the host builder gives a matrix, for the CPU tests that look at it (tests/test_wide_tile_cpu.py):
// info[0..9] = tile width, tiles, stream_len, light_len, p_len, code bits (0: raw words), words of obase, words of
// fmask (0: a narrow layout), work items, a 64-bit FNV-1a hash over every array of the layout (two layouts with the
// same bytes hash alike).  tcol / obase / fmask (each may be NULL) get up to cap_* elements of those arrays; describe
// (cap_describe bytes) the string sh_csr_describe would print for the layout.  0, or -1: the builder refused.
extern "C" int sh_debug_plan_layout(int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                    const sh_plan_options *opt_p, int n_cus, int64_t *info, uint16_t *tcol, int64_t cap_tcol, uint32_t *obase,
                                    int64_t cap_obase, uint64_t *fmask, int64_t cap_fmask, char *describe, int64_t cap_describe) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  TiledHost H;
  if (!build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, n_cus, H)) return -1;
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) { for (size_t k = 0; k < n; k++) { h ^= ((const uint8_t *)p)[k]; h *= 1099511628211ull; } };
  mix(H.bins.data(), H.bins.size() * sizeof(RowBin)); mix(H.chunks.data(), H.chunks.size() * sizeof(TileChunk));
  mix(H.heavy.data(), H.heavy.size() * sizeof(LongRow)); mix(H.tval.data(), H.tval.size() * 4); mix(H.gdest.data(), H.gdest.size() * 4);
  mix(H.gblk.data(), H.gblk.size() * 4); mix(H.lrp.data(), H.lrp.size() * 4); mix(H.obase.data(), H.obase.size() * 4);
  mix(H.ptab.data(), H.ptab.size() * 4); mix(H.ptile.data(), H.ptile.size() * 2); mix(H.tcode.data(), H.tcode.size());
  mix(H.vdict.data(), H.vdict.size() * 4); mix(H.tcol.data(), H.tcol.size() * 2); mix(H.pslot.data(), H.pslot.size() * 2);
  mix(H.fmask.data(), H.fmask.size() * 8);
  if (info) {
    info[0] = H.tcols; info[1] = (cols + H.tcols - 1) / H.tcols; info[2] = H.stream_len; info[3] = H.light_len; info[4] = H.p_len;
    info[5] = H.vdict.empty() ? 0 : H.code_bits; info[6] = (int64_t)H.obase.size(); info[7] = (int64_t)H.fmask.size();
    info[8] = (int64_t)H.chunks.size(); info[9] = (int64_t)h;
  }
  if (tcol) memcpy(tcol, H.tcol.data(), (size_t)std::min<int64_t>(cap_tcol, (int64_t)H.tcol.size()) * 2);
  if (obase) memcpy(obase, H.obase.data(), (size_t)std::min<int64_t>(cap_obase, (int64_t)H.obase.size()) * 4);
  if (fmask) memcpy(fmask, H.fmask.data(), (size_t)std::min<int64_t>(cap_fmask, (int64_t)H.fmask.size()) * 8);
  if (describe && cap_describe > 0)
    describe_tiled(describe, (size_t)cap_describe, cols, H.tcols, (int)H.vdict.size(), H.code_bits, H.vdict_used, (long long)H.chunks.size(),
                   (long long)H.bins.size(), (long long)H.heavy.size(), H.stream_len, H.light_entries, H.p_len,
                   opt.fold != 0 && (H.tcols != TCOLS || TCOL_FOLD != 0));
  return 0;
}
// The CSR arrays of a matrix on the device as the device builders take them, owned by `own`: NULL, or the HIP call that failed.
static const char *debug_upload_csr(DevArrays &own, int64_t rows, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx, const void *val,
                                    int32_t **d_rp, int32_t **d_ci, uint32_t **d_val) {
  if (own.alloc_exact(d_rp, (size_t)(rows + 1) * 4) != hipSuccess || own.alloc_exact(d_ci, (size_t)nnz * 4 + 32) != hipSuccess ||
      own.alloc_exact(d_val, (size_t)nnz * 4 + 32) != hipSuccess)
    return "hipMalloc";
  if (hipMemcpy(*d_rp, row_ptr, (size_t)(rows + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(*d_ci, col_idx, (size_t)nnz * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(*d_val, val, (size_t)nnz * 4, hipMemcpyHostToDevice) != hipSuccess)
    return "hipMemcpy";
  return nullptr;
}
// Builds the tiled layout of one matrix twice -- host builder and device builder -- and compares every array.
// Returns the number of arrays (or scalars) that differ, 0 = identical byte for byte; -1: the host builder refused the
// matrix, -2: the device builder refused or failed (report says why), -3: a HIP call of this function failed.
// report (cap bytes) gets one line per difference: the array, the first differing element, both values.
extern "C" int sh_debug_compare_builds(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                       const void *val, const sh_plan_options *opt_p, char *report, int64_t cap) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  std::string rep;
  auto finish = [&](int rc) { if (report && cap > 0) snprintf(report, (size_t)cap, "%s", rep.c_str()); return rc; };
  if (!e || nnz <= 0) { rep = "bad argument"; return finish(-3); }
  if (hipSetDevice(e->device) != hipSuccess) { rep = "hipSetDevice"; return finish(-3); }
  TiledHost hh, hg;
  TiledDevArrays td;
  struct Guard { TiledDevArrays &t; ~Guard() { t.release(); } } guard{td};
  DevArrays own;   // the CSR arrays on the device
  if (!build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, e->n_cus, hh)) { rep = "host builder refused"; return finish(-1); }
  int32_t *d_rp = nullptr, *d_ci = nullptr;
  uint32_t *d_val = nullptr;
  if (const char *bad = debug_upload_csr(own, rows, nnz, row_ptr, col_idx, val, &d_rp, &d_ci, &d_val)) { rep = bad; return finish(-3); }
  std::string why;
  const int g = build_tiled_plan_gpu(e->stream, rows, cols, nnz, row_ptr, d_rp, d_ci, d_val, opt, e->n_cus, hg, td, why);
  if (g != 1) { rep = "device builder: " + why; return finish(-2); }
  int diffs = 0;
  char line[256];
  auto scalar = [&](const char *name, long long a, long long b) {
    if (a != b) { snprintf(line, sizeof line, "%s: host %lld device %lld\n", name, a, b); rep += line; diffs++; }
  };
  scalar("stream_len", hh.stream_len, hg.stream_len); scalar("p_len", hh.p_len, hg.p_len); scalar("light_len", hh.light_len, hg.light_len);
  scalar("heavy_base", hh.heavy_base, hg.heavy_base); scalar("light_entries", hh.light_entries, hg.light_entries);
  scalar("n_partials", hh.n_partials, hg.n_partials); scalar("code_bits", hh.code_bits, hg.code_bits); scalar("vdict_used", hh.vdict_used, hg.vdict_used);
  scalar("n_bins", (long long)hh.bins.size(), (long long)hg.bins.size()); scalar("n_chunks", (long long)hh.chunks.size(), (long long)hg.chunks.size());
  scalar("n_heavy", (long long)hh.heavy.size(), (long long)hg.heavy.size()); scalar("tcols", hh.tcols, hg.tcols);
  scalar("tile_fill*1e6", (long long)(hh.tile_fill * 1e6), (long long)(hg.tile_fill * 1e6));
  auto host_bytes = [&](const char *name, const void *a, size_t na, const void *b, size_t nb, size_t elem) {
    if (na != nb) { snprintf(line, sizeof line, "%s: %zu vs %zu bytes\n", name, na, nb); rep += line; diffs++; return; }
    if (na && memcmp(a, b, na) != 0) {
      size_t k = 0;
      while (k < na && ((const uint8_t *)a)[k] == ((const uint8_t *)b)[k]) k++;
      size_t ndiff = 0;
      for (size_t q = 0; q + elem <= na; q += elem) if (memcmp((const uint8_t *)a + q, (const uint8_t *)b + q, elem) != 0) ndiff++;
      const size_t el = k / elem;
      unsigned long long va = 0, vb = 0;
      memcpy(&va, (const uint8_t *)a + el * elem, std::min<size_t>(elem, 8)); memcpy(&vb, (const uint8_t *)b + el * elem, std::min<size_t>(elem, 8));
      snprintf(line, sizeof line, "%s: %zu of %zu elements differ, first at %zu: host 0x%llx device 0x%llx\n", name, ndiff, na / elem, el, va, vb);
      rep += line; diffs++;
    }
  };
  host_bytes("bins", hh.bins.data(), hh.bins.size() * sizeof(RowBin), hg.bins.data(), hg.bins.size() * sizeof(RowBin), sizeof(RowBin));
  host_bytes("chunks", hh.chunks.data(), hh.chunks.size() * sizeof(TileChunk), hg.chunks.data(), hg.chunks.size() * sizeof(TileChunk), sizeof(TileChunk));
  host_bytes("heavy", hh.heavy.data(), hh.heavy.size() * sizeof(LongRow), hg.heavy.data(), hg.heavy.size() * sizeof(LongRow), sizeof(LongRow));
  host_bytes("vdict", hh.vdict.data(), hh.vdict.size() * 4, hg.vdict.data(), hg.vdict.size() * 4, 4);
  bool hip_ok = true;
  auto dev_bytes = [&](const char *name, const void *host, size_t nbytes_host, const void *dev, size_t n_dev, size_t elem) {
    std::vector<uint8_t> tmp(n_dev * elem);
    if (n_dev && hipMemcpy(tmp.data(), dev, n_dev * elem, hipMemcpyDeviceToHost) != hipSuccess) { hip_ok = false; return; }
    host_bytes(name, host, nbytes_host, tmp.data(), n_dev * elem, elem);
  };
  dev_bytes("lrp", hh.lrp.data(), hh.lrp.size() * 4, td.lrp, td.n_lrp, 4);
  dev_bytes("tcol", hh.tcol.data(), hh.tcol.size() * 2, td.tcol, td.n_tcol, 2);
  dev_bytes("tcode", hh.tcode.data(), hh.tcode.size(), td.tcode, td.n_tcode, 1);
  dev_bytes("tval", hh.tval.data(), hh.tval.size() * 4, td.tval, td.n_tval, 4);
  dev_bytes("gdest", hh.gdest.data(), hh.gdest.size() * 4, td.gdest, td.n_gdest, 4);
  dev_bytes("pslot", hh.pslot.data(), hh.pslot.size() * 2, td.pslot, td.n_pslot, 2);
  dev_bytes("gblk", hh.gblk.data(), hh.gblk.size() * 4, td.gblk, td.n_gblk, 4);
  dev_bytes("ptab", hh.ptab.data(), hh.ptab.size() * 4, td.ptab, td.n_ptab, 4);
  dev_bytes("ptile", hh.ptile.data(), hh.ptile.size() * 2, td.ptile, td.n_ptab, 2);
  dev_bytes("obase", hh.obase.data(), hh.obase.size() * 4, td.obase, td.n_obase, 4);
  dev_bytes("fmask", hh.fmask.data(), hh.fmask.size() * 8, td.fmask, td.n_fmask, 8);
  if (!hip_ok) { rep += "hipMemcpy (download) failed\n"; return finish(-3); }
  return finish(diffs);
}
// The limit on the products in P (plan_common.h::max_p_len) for the tests: products > 0 lowers it to that many products,
// 0 restores the real one, a negative value changes nothing.  Returns the REAL bound (the constant of the product build).
extern "C" int64_t sh_debug_set_p_limit(int64_t products) {
  if (products >= 0) g_debug_p_limit = products;
  return P_LEN_MAX;
}
// Makes the NEXT call of build_tiled_plan_gpu report a failed device step (-1, why = "injected"): where = 1 before its
// first allocation, where = 2 immediately before it would return 1 (the layout complete, the big arrays in
// TiledDevArrays, TiledHost filled, the stream idle); 0 turns it off.  A host-side switch: no launched kernel changes.
// It applies to one call and clears itself.
extern "C" void sh_debug_fail_device_build(int where) { g_debug_fail_device_build = where; }
// How many arrays of an abandoned device build sh_csr_upload_ex still held when it last started the host builder (a
// fallback releases them first: the host-built layout must not need room beside them).
extern "C" int sh_debug_held_at_host_build(void) { return g_debug_held_at_host_build; }
// Both builders run independently on one matrix: *host_verdict = 1 built / 0 refused, *device_verdict = 1 built /
// 0 refused / -1 a device step failed, `why` (cap bytes) = what the device builder said.  Everything made here is freed
// before it returns.  0, or -3 when a HIP call of this function itself failed (why then names it).
extern "C" int sh_debug_build_verdicts(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr, const int32_t *col_idx,
                                       const void *val, const sh_plan_options *opt_p, int32_t *host_verdict, int32_t *device_verdict,
                                       char *why_out, int64_t cap) {
  sh_plan_options opt;
  if (opt_p) opt = *opt_p; else sh_plan_options_default(&opt);
  std::string why;
  auto finish = [&](int rc) { if (why_out && cap > 0) snprintf(why_out, (size_t)cap, "%s", why.c_str()); return rc; };
  if (!e || nnz <= 0 || rows <= 0 || !host_verdict || !device_verdict) { why = "bad argument"; return finish(-3); }
  if (hipSetDevice(e->device) != hipSuccess) { why = "hipSetDevice"; return finish(-3); }
  {
    TiledHost hh;
    *host_verdict = build_tiled_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, e->n_cus, hh) ? 1 : 0;
  }
  TiledHost hg;
  TiledDevArrays td;
  struct Guard { TiledDevArrays &t; ~Guard() { t.release(); } } guard{td};
  DevArrays own;   // the CSR arrays on the device
  int32_t *d_rp = nullptr, *d_ci = nullptr;
  uint32_t *d_val = nullptr;
  if (const char *bad = debug_upload_csr(own, rows, nnz, row_ptr, col_idx, val, &d_rp, &d_ci, &d_val)) { why = bad; return finish(-3); }
  *device_verdict = build_tiled_plan_gpu(e->stream, rows, cols, nnz, row_ptr, d_rp, d_ci, d_val, opt, e->n_cus, hg, td, why);
  if (hipStreamSynchronize(e->stream) != hipSuccess) { why = "hipStreamSynchronize"; return finish(-3); }
  return finish(0);
}
// The bit-blocked (or,and) layout built by both builders and compared: 0 = identical, else the number of differing
// arrays; -1 host refused, -2 device refused / failed, -3 HIP error here.
extern "C" int sh_debug_compare_bits_builds(sh_engine *e, int64_t rows, int64_t cols, int64_t nnz, const int32_t *row_ptr,
                                            const int32_t *col_idx, const void *val, char *report, int64_t cap) {
  std::string rep;
  auto finish = [&](int rc) { if (report && cap > 0) snprintf(report, (size_t)cap, "%s", rep.c_str()); return rc; };
  if (!e || nnz <= 0) { rep = "bad argument"; return finish(-3); }
  if (hipSetDevice(e->device) != hipSuccess) { rep = "hipSetDevice"; return finish(-3); }
  sh_plan_options opt;
  sh_plan_options_default(&opt);
  BitsHost hh, hg;
  if (!build_bits_plan(rows, cols, nnz, row_ptr, col_idx, (const uint32_t *)val, opt, hh)) { rep = "host builder refused"; return finish(-1); }
  DevArrays own;   // the CSR arrays and the entry array on the device
  int32_t *d_rp = nullptr, *d_ci = nullptr;
  uint32_t *d_val = nullptr, *d_ent = nullptr;
  if (const char *bad = debug_upload_csr(own, rows, nnz, row_ptr, col_idx, val, &d_rp, &d_ci, &d_val)) { rep = bad; return finish(-3); }
  std::string why;
  if (build_bits_plan_gpu(e->stream, rows, cols, nnz, d_rp, d_ci, d_val, hg, &d_ent, why) != 1) { rep = "device builder: " + why; return finish(-2); }
  own.adopt(d_ent, (size_t)hg.ent_len * 4 + SLACK_WIDE);
  int diffs = 0;
  char line[256];
  auto same = [&](const char *name, const void *a, size_t na, const void *b, size_t nb) {
    if (na != nb || (na && memcmp(a, b, na) != 0)) {
      size_t k = 0;
      while (k < std::min(na, nb) && ((const uint8_t *)a)[k] == ((const uint8_t *)b)[k]) k++;
      snprintf(line, sizeof line, "%s: %zu vs %zu bytes, first difference at byte %zu\n", name, na, nb, k);
      rep += line; diffs++;
    }
  };
  std::vector<uint32_t> ent((size_t)hg.ent_len);
  if (hipMemcpy(ent.data(), d_ent, ent.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { rep = "hipMemcpy (download)"; return finish(-3); }
  same("ent", hh.ent.data(), hh.ent.size() * 4, ent.data(), ent.size() * 4);
  same("items", hh.items.data(), hh.items.size() * sizeof(BitsItem), hg.items.data(), hg.items.size() * sizeof(BitsItem));
  same("bsub", hh.bsub.data(), hh.bsub.size() * 4, hg.bsub.data(), hg.bsub.size() * 4);
  same("rr_item0", hh.rr_item0.data(), hh.rr_item0.size() * 4, hg.rr_item0.data(), hg.rr_item0.size() * 4);
  if (hh.entries != hg.entries || hh.n_rr != hg.n_rr || hh.n_ct != hg.n_ct || hh.ent_len != hg.ent_len) { rep += "scalars differ\n"; diffs++; }
  return finish(diffs);
}

// Placement experiments (tools/placement_probe.py): move one array of the tiled plan to a fresh allocation (hold != 0:
// the old one is kept allocated -- and leaked until process exit -- so that the new one cannot land in the same place),
// return its new address.  which: 0 P, 1 tcol, 2 tcode / tval, 3 pslot, 4 gblk, 5 ptab, 6 obase, 7 lrp.
// align_log2 > 21: the new place is the first address aligned to 2^align_log2 inside an allocation that much larger (the
// base is leaked: experiments only).
extern "C" int sh_debug_move_array(sh_engine *e, sh_csr *m, int which, int hold, int align_log2, uint64_t *address) {
  if (!e || !m || m->plan != PLAN_TILED) return SH_EINVAL;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return SH_EHIP;
  TiledLayout &t = m->tiled;
  void **slot = nullptr;
  switch (which) {
    case 0: slot = (void **)&t.d_P; break;
    case 1: slot = (void **)&t.d_tcol; break;
    case 2: slot = t.n_vdict ? (void **)&t.d_tcode : (void **)&t.d_tval; break;
    case 3: slot = (void **)&t.d_pslot; break;
    default: return SH_EINVAL;
  }
  const size_t bytes = t.dev.size_of(*slot);   // (as allocated at upload, slack included)
  void *fresh = nullptr;
  const size_t align = align_log2 > 21 ? (size_t)1 << align_log2 : 0;
  if (hipMalloc(&fresh, bytes + align) != hipSuccess) return SH_ENOMEM;
  if (align) fresh = (void *)(((uintptr_t)fresh + align - 1) & ~(uintptr_t)(align - 1));
  if (hipMemcpy(fresh, *slot, bytes, hipMemcpyDeviceToDevice) != hipSuccess) return SH_EHIP;
  t.dev.replace(*slot, fresh);
  if (!hold) (void)hipFree(*slot);
  *slot = fresh;
  if (address) *address = (uint64_t)(uintptr_t)fresh;
  return SH_OK;
}
// (placement experiments) point the matrix at another product array allocated by sh_debug_move_array(which = 0, hold = 1);
// its own stays with its layout, the other one with the matrix that moved to it
extern "C" int sh_debug_set_P(sh_engine *e, sh_csr *m, uint64_t address) {
  if (!e || !m || m->plan != PLAN_TILED || !address) return SH_EINVAL;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return SH_EHIP;
  m->tiled.d_P = (uint32_t *)(uintptr_t)address;
  return SH_OK;
}
// Launch hygiene (tests/test_hygiene_gpu.py): what a launch may read is what it wrote itself.  Drains the stream, then
// fills the per-launch scratch of every layout the matrix holds -- data words and flags only, never a word that is read
// as an address: data_word into P (the identity group behind the products included), the heavy rows' partials, the
// long-row partials of the stream plan and the bitmap and partials of the bit-blocked layout; live_word into the
// tiles' live words; PIECE_DEAD (which phase 2 handles in bounds) into the marked piece table when dead_piece != 0.
// sizes[0..7]: the bytes filled of P, tpartial, tile_live, ptab_live, partial, partial_multi, xbits, bits_partial
// (0: the matrix has no such array).
extern "C" int sh_debug_poison_scratch(sh_engine *e, sh_csr *m, uint32_t data_word, uint32_t live_word, int dead_piece, int64_t *sizes) {
  if (!e || !m || !sizes) return SH_EINVAL;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return SH_EHIP;
  bool ok = true;
  auto fill = [&](void *p, size_t bytes, uint32_t word) -> int64_t {
    if (!p || bytes < 4) return 0;
    ok = ok && hipMemsetD32Async((hipDeviceptr_t)p, (int)word, bytes / 4, e->stream) == hipSuccess;
    return (int64_t)(bytes / 4 * 4);
  };
  const TiledLayout &t = m->tiled;
  const StreamLayout &s = m->stream;
  const BitsLayout &b = m->bits;
  sizes[0] = fill(t.d_P, t.dev.size_of(t.d_P), data_word);
  sizes[1] = fill(t.d_tpartial, t.dev.size_of(t.d_tpartial), data_word);
  sizes[2] = fill(t.d_tile_live, t.dev.size_of(t.d_tile_live), live_word);
  sizes[3] = dead_piece ? fill(t.d_ptab_live, t.d_ptab_live ? (size_t)t.n_pieces * 4 : 0, (uint32_t)PIECE_DEAD) : 0;
  sizes[4] = fill(s.d_partial, s.dev.size_of(s.d_partial), data_word);
  sizes[5] = fill(s.d_partial_multi, s.dev.size_of(s.d_partial_multi), data_word);
  sizes[6] = fill(b.d_xbits, b.dev.size_of(b.d_xbits), data_word);
  sizes[7] = fill(b.d_bits_partial, b.dev.size_of(b.d_bits_partial), data_word);
  return ok && hipStreamSynchronize(e->stream) == hipSuccess ? SH_OK : SH_EHIP;
}
// ... and the device halves of the words a batch of dense launches writes (DenseLoopState), those that a loop has opened
// so far.  sizes[0..2]: the bytes filled of flags, mflags, bstate (0: not open yet).
extern "C" int sh_debug_poison_loop_words(sh_engine *e, uint32_t word, int64_t *sizes) {
  if (!e || !sizes) return SH_EINVAL;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return SH_EHIP;
  bool ok = true;
  auto fill = [&](void *d, size_t bytes) -> int64_t {
    if (!d || bytes < 4) return 0;
    ok = ok && hipMemsetD32Async((hipDeviceptr_t)d, (int)word, bytes / 4, e->stream) == hipSuccess;
    return (int64_t)(bytes / 4 * 4);
  };
  sizes[0] = fill(e->dense.flags.d, e->dense.flags.size);
  sizes[1] = fill(e->dense.mflags.d, e->dense.mflags.size);
  sizes[2] = fill(e->dense.bstate.d, e->dense.bstate.size);
  return ok && hipStreamSynchronize(e->stream) == hipSuccess ? SH_OK : SH_EHIP;
}
// (slab experiments, tools/slab_probe.py) words of the matrix's product array, for a host-side bounds check before matrices share one
extern "C" int64_t sh_debug_p_len(const sh_csr *m) { return m && m->plan == PLAN_TILED ? m->tiled.p_len : -1; }
