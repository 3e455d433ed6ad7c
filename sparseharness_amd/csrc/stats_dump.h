// stats_dump.h -- included by engine.hip under -DSH_STATS only (experiments; never the product build): with SH_STATS_DUMP
// set, launch_tiled prints where phase 1's chunks and the two roles of phase 2 spent their time (counters of kernels.hip.h).
#pragma once
static uint64_t *g_p1_stats_buf = nullptr;   // per-chunk timeline of phase 1

// In front of phase 1: the timeline is cleared and the kernels are pointed at it.
static void stats_before_tiled(sh_engine *e) {
  if (!getenv("SH_STATS_DUMP")) return;
  if (!g_p1_stats_buf) (void)hipMalloc((void **)&g_p1_stats_buf, (size_t)1 << 22);
  (void)hipMemsetAsync(g_p1_stats_buf, 0, (size_t)1 << 22, e->stream);
  (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_p1_stats), &g_p1_stats_buf, sizeof g_p1_stats_buf, 0, hipMemcpyHostToDevice, e->stream);
}

// Behind phase 2.
static void stats_after_tiled(sh_engine *e, int n_bins, int n_chunks) {
  if (!getenv("SH_STATS_DUMP")) return;
  if (n_bins > 0) {   // where the two roles of phase 2 spent their cycles (wave 0 of each role, per workgroup)
    (void)hipStreamSynchronize(e->stream);
    std::vector<uint64_t> pf(256 * 16);
    (void)hipMemcpyFromSymbol(pf.data(), HIP_SYMBOL(g_p2_prof), pf.size() * 8);
    const int G = std::min(n_bins, 256);
    double a[16] = {0};
    for (int w = 0; w < G; w++) for (int k = 0; k < 16; k++) a[k] += (double)pf[(size_t)w * 16 + k] / G;
    fprintf(stderr, "[stats] phase 2 per workgroup (%d, %.1f bins each), shader cycles: loaders total %.0f, in vmcnt waits %.0f (%.1f %%), in barriers %.0f (%.1f %%), issuing/scattering %.0f | "
                    "reducers total %.0f, in barriers %.0f (%.1f %%), reducing %.0f (one-lane pass %.0f, 8-lane rows %.0f, 64-lane rows %.0f)\n",
            G, a[3], a[0], a[1], 100 * a[1] / a[0], a[2], 100 * a[2] / a[0], a[0] - a[1] - a[2], a[4], a[5], 100 * a[5] / a[4], a[6], a[8], a[9], a[10]);
    // the same per reducer wave: who a bin waits for
    std::vector<uint64_t> pw(256 * 12 * 4);
    (void)hipMemcpyFromSymbol(pw.data(), HIP_SYMBOL(g_p2_wave), pw.size() * 8);
    fprintf(stderr, "[stats] phase 2 reducer waves (K cycles: at barriers / classifying pass / cooperative rows / total):");
    for (int w = 0; w < 12; w++) {
      double a[4] = {0, 0, 0, 0};
      for (int g = 0; g < G; g++) for (int k = 0; k < 4; k++) a[k] += (double)pw[((size_t)g * 12 + w) * 4 + k] / G;
      fprintf(stderr, "  w%d %.0f/%.0f/%.0f/%.0f", w, a[0] / 1e3, a[1] / 1e3, a[2] / 1e3, a[3] / 1e3);
    }
    fprintf(stderr, "\n");
  }
  if (g_p1_stats_buf) {
    const int nch = n_chunks;
    std::vector<uint64_t> hs((size_t)nch * 5);
    (void)hipStreamSynchronize(e->stream);
    (void)hipMemcpy(hs.data(), g_p1_stats_buf, hs.size() * 8, hipMemcpyDeviceToHost);
    // SH_STATS_P1_FILE=path: the records themselves, one line per work item of this launch (the file holds the last
    // launch; tools/p1_timeline.py turns it into the per-XCD summary).  Block b runs on XCD b % 8.
    if (const char *path = getenv("SH_STATS_P1_FILE")) {
      if (FILE *f = fopen(path, "w")) {
        fprintf(f, "block,kind,entries,start,staged,end\n");
        for (int i = 0; i < nch; i++) {
          const uint64_t *S = &hs[(size_t)i * 5];
          if (S[1] == 0) continue;   // a filler
          fprintf(f, "%d,%d,%llu,%llu,%llu,%llu\n", i, (int)S[0], (unsigned long long)S[1], (unsigned long long)S[2],
                  (unsigned long long)S[3], (unsigned long long)S[4]);
        }
        fclose(f);
      }
    }
    for (int kind = 0; kind < 2; kind++) {
      double n = 0, ent = 0, stage = 0, total = 0;
      uint64_t t0 = ~0ull, t1 = 0;
      for (int i = 0; i < nch; i++) {
        const uint64_t *S = &hs[(size_t)i * 5];
        if (S[1] == 0 || (int)S[0] != kind) continue;
        n++; ent += S[1]; stage += (S[3] - S[2]) / 100.0; total += (S[4] - S[2]) / 100.0;
        t0 = std::min(t0, S[2]); t1 = std::max(t1, S[4]);
      }
      if (n > 0)
        fprintf(stderr, "[stats] phase 1 %s chunks: %.0f, %.0f entries each, staging %.2f us, whole chunk %.2f us (incl. store drain); span %.1f us\n",
                kind ? "heavy" : "light", n, ent / n, stage / n, total / n, (t1 - t0) / 100.0);
    }
  }
}
