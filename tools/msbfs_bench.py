#!/usr/bin/env python3
"""What packing 32 BFS sources into a word buys: for one matrix and each `words` in {1, 2, 4, 8} it runs
sh_bits_iterate (alpha = 1, beta = 1) from 32 * words seeded random sources to convergence and records the total
device time and the launches.  In the same process, alternating with it, the two ways a caller has today:

  (a) sh_iterate(SH_OR_AND_I32) from ONE source under the plan sh_csr_upload chooses by default, on a seeded sample of
      `--sample` (>= 8) of those sources; the mean over the sample of each source's median run, times 32 * words, is
      what that many single-source runs cost (the sources differ: an isolated vertex is confirmed by one launch);
  (b) sh_iterate_multi(SH_OR_AND_I32, width 32) on the plan = 1 matrix from the first 32 sources, times `words`.

Method: every figure is device time between events on the engine's stream (the total_ns of the C ABI: the sum over
the launches of a run); per `words`, one warm-up of each kind, then `--rounds` rounds of {sh_bits_iterate,
sh_iterate_multi, the sampled sh_iterate runs}; medians over the rounds, the spread (min, max) beside them.
Before timing, bit s of the packed result is compared with the single-source result for every sampled source, and
the launch counts with them.

  python tools/msbfs_bench.py --matrix synth:scircuit --out profiles/msbfs_scircuit.json
  python tools/msbfs_bench.py --matrix synth:rmat-23
  python tools/msbfs_bench.py --matrix synth:powerlaw-10000000-200000000 --rounds 3

One JSON object on stdout (and in --out).  `calls` counts the calls and launches made, for a kernel trace to be held against.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparseharness_amd import hostlib as H  # noqa: E402
from sparseharness_amd.engine import OR_AND_I32, Engine  # noqa: E402


def load_matrix(spec):
    if spec.startswith("synth:"):
        kind = spec[len("synth:"):]
        if kind == "scircuit":
            rp, ci, va = H.scircuit_like()
            return 170_998, rp, ci, va
        if kind.startswith("rmat-"):
            scale = int(kind.split("-")[1])
            rp, ci, va = H.rmat(scale)
            return 1 << scale, rp, ci, va
        if kind.startswith("powerlaw-"):
            _, rows, nnz = kind.split("-")
            rp, ci, va = H.powerlaw(int(rows), int(nnz))
            return int(rows), rp, ci, va
        raise SystemExit(f"unknown generator {spec}: synth:scircuit | synth:rmat-<scale> | synth:powerlaw-<rows>-<entries>")
    rows, cols, _, rp, ci, va = H.mm_load(spec, elem_is_int=True)
    if rows != cols:
        raise SystemExit("the iteration needs a square matrix")
    return rows, rp, ci, va


def summary(ns):
    us = sorted(v / 1e3 for v in ns)
    return {"median_us": round(statistics.median(us), 3), "min_us": round(us[0], 3), "max_us": round(us[-1], 3), "n": len(us)}


def packed_start(n, words, sources):
    P = np.zeros((n, words), np.uint32)
    for s, v in enumerate(sources):
        P[v, s // 32] |= np.uint32(1) << np.uint32(s % 32)
    return P


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--words", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample", type=int, default=8, help="single-source runs per round (at least 8)")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.sample < 8:
        raise SystemExit("--sample: at least 8")
    words_list = [int(w) for w in args.words.split(",")]

    n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va).astype(np.int32)   # the BFS app's integer matrix (every stored value != 0 stays != 0)
    cap = args.max_iters
    res = {"tool": "tools/msbfs_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "semiring": "or_and_i32",
           "alpha": 1, "beta": 1, "rounds": args.rounds, "sample": args.sample, "max_iters": cap,
           "timing": "device events around each launch (total_ns of the C ABI); medians over the rounds",
           "comparators": {"single": "32 * words x mean over a seeded sample of the sources of the source's median sh_iterate run (default plan)",
                           "multi32": "words x sh_iterate_multi at width 32 on the plan = 1 matrix (first 32 sources)"},
           "words": {}, "calls": {"sh_bits_iterate": 0, "packed_launches": 0, "sh_iterate": 0, "sh_iterate_multi": 0}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        A_def = eng.upload_csr(n, n, rp, ci, va)            # what sh_csr_upload chooses (the environment included)
        A_str = eng.upload_csr(n, n, rp, ci, va, plan=1)    # the CSR-stream plan: what the packed kernels run on
        res["default_plan"] = A_def.describe()
        res["stream_plan"] = A_str.describe()
        x1, y1, s1 = eng.alloc(n), eng.alloc(n), eng.alloc(n)
        for W in words_list:
            n_src = 32 * W
            rng = np.random.default_rng(1000 + W)
            sources = [int(v) for v in rng.choice(n, n_src, replace=False)]
            sample = [int(j) for j in rng.choice(n_src, args.sample, replace=False)]
            P0 = packed_start(n, W, sources)
            M0 = np.zeros((n, 32), np.int32)
            M0[sources[:32], np.arange(32)] = 1
            Xb, Yb, Sb = eng.alloc(n * W), eng.alloc(n * W), eng.alloc(n * W)
            Xm, Ym, Sm = eng.alloc(n * 32), eng.alloc(n * 32), eng.alloc(n * 32)

            def run_bits():
                Xb.upload(P0)
                Yb.upload(P0)
                r = eng.bits_iterate(A_str, Xb, Yb, Sb, 1, 1, W, max_iters=cap)
                res["calls"]["sh_bits_iterate"] += 1
                res["calls"]["packed_launches"] += r[0]
                return r

            def run_multi():
                Xm.upload(M0)
                Ym.upload(M0)
                res["calls"]["sh_iterate_multi"] += 1
                return eng.iterate_multi(OR_AND_I32, A_str, Xm, Ym, Sm, 1, 1, 32, max_iters=cap)

            def run_single(j):
                x0 = np.zeros(n, np.int32)
                x0[sources[j]] = 1
                x1.upload(x0)
                y1.upload(x0)
                res["calls"]["sh_iterate"] += 1
                return eng.iterate(OR_AND_I32, A_def, x1, y1, s1, 1, 1, max_iters=cap)

            # warm-up of each kind, and the check: bit s == the single-source run, for the sampled sources
            launches, iters, conv, _, _ = run_bits()
            got = Xb.download(np.uint32, shape=(n, W))
            run_multi()
            for j in sample:
                it, cv, _, _ = run_single(j)
                bit = ((got[:, j // 32] >> np.uint32(j % 32)) & np.uint32(1)).astype(np.int32)
                if not np.array_equal(bit, (x1.download(np.int32) != 0).astype(np.int32)) or (iters[j], conv[j]) != (it, cv):
                    raise SystemExit(f"words {W}: source bit {j} (vertex {sources[j]}) differs from sh_iterate")
            t_bits, t_multi, t_single = [], [], {j: [] for j in sample}
            m_launches = 0
            for _ in range(args.rounds):
                t_bits.append(run_bits()[4])
                r = run_multi()
                m_launches = r[0]
                t_multi.append(r[4])
                for j in sample:
                    t_single[j].append(run_single(j)[3])
            sb, sm, ss = summary(t_bits), summary(t_multi), summary([t for v in t_single.values() for t in v])
            # a source's time is the median of its runs; the sources differ (an isolated vertex is confirmed by one launch,
            # another needs ten), so what 32 * words of them cost is 32 * words times the MEAN over the sample
            per_source_us = [statistics.median(v) / 1e3 for v in t_single.values()]
            single_us = statistics.fmean(per_source_us)
            res["words"][str(W)] = {
                "sources": n_src, "launches": launches, "launches_per_source_min_max": [min(iters), max(iters)],
                "all_converged": all(conv), "t_bits_iterate": sb, "us_per_launch": round(sb["median_us"] / max(launches, 1), 3),
                "t_iterate_multi_width32": sm, "launches_iterate_multi": m_launches, "t_iterate_single_default_plan": ss,
                "single_us_per_sampled_source": [round(t, 3) for t in per_source_us], "single_mean_us": round(single_us, 3),
                "single_launches_per_sampled_source": [iters[j] for j in sample],
                "ratio_vs_single": round(sb["median_us"] / (n_src * single_us), 5),
                "ratio_vs_multi32": round(sb["median_us"] / (W * sm["median_us"]), 5),
                "us_per_source": round(sb["median_us"] / n_src, 3),
                # by construction: the 8-byte entry and the 4 * words gathered bytes are shared by 32 * words sources
                "bytes_per_entry_per_source_by_construction": round((8.0 + 4.0 * W) / n_src, 4),
                "gathers_per_entry_per_source_by_construction": round(1.0 / n_src, 5) if W <= 4 else round(2.0 / n_src, 5),
                "x_bytes": n * W * 4, "checked_sources": len(sample),
            }
            print(f"words {W}: {json.dumps(res['words'][str(W)])}", file=sys.stderr, flush=True)
            for v in (Xb, Yb, Sb, Xm, Ym, Sm):
                v.free()
        A_def.free()
        A_str.free()
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
