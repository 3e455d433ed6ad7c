#!/usr/bin/env python3
"""What reading the matrix once for K vectors buys: for one matrix and each K it times sh_spmm and, in the same process
and alternating with it, sh_spmv on the same matrix -- under the plan sh_csr_upload chooses by default and under the
CSR-stream plan -- and reports t_spmm(K) / (K * t_spmv).  The single-vector path is the comparator: K launches of it
are what a caller pays today for K vectors.

Method: every figure is the device time of one call between two events on the engine's stream (the `kernel_ns` of the
C ABI); per K, `--rounds` rounds of {`--reps` x sh_spmm, `--reps` x sh_spmv default plan, `--reps` x sh_spmv stream
plan} after warm-up launches of each; the medians over all rounds are reported, and the spread (min, max) beside them.
(+,x), alpha = 1, beta = 0, x drawn from [0.5, 1.5).  Before timing, column 0 of one sh_spmm is compared with sh_spmv
on the same vector (relative 1e-5: the two sum a row in different orders).

  python tools/spmm_bench.py --matrix synth:scircuit --out profiles/spmm_scircuit.json
  python tools/spmm_bench.py --matrix synth:rmat-23
  python tools/spmm_bench.py --matrix synth:powerlaw-10000000-200000000 --widths 4,8
  python tools/spmm_bench.py --matrix tests/golden/matrix2.mtx

One JSON object on stdout (and in --out).  `calls` counts the sh_spmm calls made, for a kernel trace to be held against.
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
from sparseharness_amd.engine import PLUS_TIMES_F32, Engine  # noqa: E402


def load_matrix(spec):
    if spec.startswith("synth:"):
        kind = spec[len("synth:"):]
        if kind == "scircuit":
            rp, ci, va = H.scircuit_like()
            return 170_998, 170_998, rp, ci, va
        if kind.startswith("rmat-"):
            scale = int(kind.split("-")[1])
            rp, ci, va = H.rmat(scale)
            return 1 << scale, 1 << scale, rp, ci, va
        if kind.startswith("powerlaw-"):
            _, rows, nnz = kind.split("-")
            rp, ci, va = H.powerlaw(int(rows), int(nnz))
            return int(rows), int(rows), rp, ci, va
        raise SystemExit(f"unknown generator {spec}: synth:scircuit | synth:rmat-<scale> | synth:powerlaw-<rows>-<entries>")
    rows, cols, _, rp, ci, va = H.mm_load(spec)
    return rows, cols, rp, ci, va


def summary(ns):
    us = sorted(v / 1e3 for v in ns)
    return {"median_us": round(statistics.median(us), 3), "min_us": round(us[0], 3), "max_us": round(us[-1], 3), "n": len(us)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--widths", default="4,8,16,32")
    ap.add_argument("--reps", type=int, default=10, help="timed calls of each kind per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]

    rows, cols, rp, ci, va = load_matrix(args.matrix)
    nnz = int(rp[-1])
    rng = np.random.default_rng(2024)
    res = {"tool": "tools/spmm_bench.py", "matrix": args.matrix, "rows": rows, "cols": cols, "entries": nnz,
           "semiring": "plus_times_f32", "reps": args.reps, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "device events around each call (kernel_ns of the C ABI); medians over rounds x reps calls",
           "comparator": "width x median sh_spmv on the same matrix in the same process (default plan; stream plan beside it)",
           "widths": {}, "calls": {"sh_spmm": 0, "sh_spmv": 0}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        A_def = eng.upload_csr(rows, cols, rp, ci, va)            # what sh_csr_upload chooses (the environment included)
        A_str = eng.upload_csr(rows, cols, rp, ci, va, plan=1)    # the CSR-stream plan: what sh_spmm runs on
        res["default_plan"] = A_def.describe()
        res["stream_plan"] = A_str.describe()
        x1 = rng.uniform(0.5, 1.5, cols).astype(np.float32)
        xv, ov = eng.vector(x1), eng.alloc(rows)
        for K in widths:
            X = rng.uniform(0.5, 1.5, (cols, K)).astype(np.float32)
            X[:, 0] = x1
            Xv, Ov = eng.vector(X), eng.alloc(rows * K)
            # same numbers as the single-vector path
            eng.spmm(PLUS_TIMES_F32, A_str, Xv, None, 1.0, 0.0, Ov, K)
            eng.spmv(PLUS_TIMES_F32, A_str, xv, None, 1.0, 0.0, ov)
            res["calls"]["sh_spmm"] += 1
            res["calls"]["sh_spmv"] += 1
            got, want = Ov.download(np.float32, shape=(rows, K))[:, 0].astype(np.float64), ov.download(np.float32).astype(np.float64)
            worst = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if rows else 0.0
            if worst > 1e-5:
                raise SystemExit(f"width {K}: column 0 of sh_spmm is {worst:.3e} (relative) off sh_spmv")
            kinds = {
                "spmm": lambda: eng.spmm(PLUS_TIMES_F32, A_str, Xv, None, 1.0, 0.0, Ov, K, timed=True),
                "spmv_default": lambda: eng.spmv(PLUS_TIMES_F32, A_def, xv, None, 1.0, 0.0, ov, timed=True),
                "spmv_stream": lambda: eng.spmv(PLUS_TIMES_F32, A_str, xv, None, 1.0, 0.0, ov, timed=True),
            }
            ns = {k: [] for k in kinds}
            for k, fn in kinds.items():
                for _ in range(args.warmup):
                    fn()
                    res["calls"]["sh_spmm" if k == "spmm" else "sh_spmv"] += 1
            for _ in range(args.rounds):
                for k, fn in kinds.items():
                    for _ in range(args.reps):
                        ns[k].append(fn())
                        res["calls"]["sh_spmm" if k == "spmm" else "sh_spmv"] += 1
            s = {k: summary(v) for k, v in ns.items()}
            t = s["spmm"]["median_us"]
            res["widths"][str(K)] = {
                "t_spmm": s["spmm"], "t_spmv_default_plan": s["spmv_default"], "t_spmv_stream_plan": s["spmv_stream"],
                "ratio_vs_default_plan": round(t / (K * s["spmv_default"]["median_us"]), 4),
                "ratio_vs_stream_plan": round(t / (K * s["spmv_stream"]["median_us"]), 4),
                "us_per_vector": round(t / K, 3),
                # by construction: the 8-byte entry shared by K vectors + the 4-byte x word each of them gathers
                "bytes_per_entry_per_vector_by_construction": round(8.0 / K + 4.0, 3),
                "x_bytes": cols * K * 4,
                "worst_relative_difference_to_sh_spmv": worst,
            }
            Xv.free()
            Ov.free()
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
