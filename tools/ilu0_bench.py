#!/usr/bin/env python3
"""What sh_ilu0 costs, for one matrix, in one process and with the arms alternating:

  sh_ilu0        device time of one float64 factorisation (the handle made once, the values given per call), for every
                 `thin` of --thin (consecutive levels of at most `thin` rows share a one-workgroup launch; 0: one launch
                 per level), with the launches, the runs and the levels those hold;
  ilu0_factor    wall time of the host's serial IKJ recurrence in the same order (hostlib.ilu0_factor) -- the baseline.

The matrix: the pattern of --matrix, symmetrised (--symmetrise) or as given, its off-diagonal entries with the value -1
and a diagonal of 1 + the entries of the row (diagonally dominant, so the factor stays bounded; synth:grid-<side>: 4, the
5-point Laplacian).  --color permutes it first by sh_color's classes (stable by colour): rows of one colour share a level.

The handle's `work` (the look-ups of one factorisation) is printed before anything is factorised: hub rows make it grow
like the wedge count, and the host gold's time grows with it.  --host-only stops after the gold: no device is needed to
learn whether a matrix is within reach.

Method: first lu of every arm is compared with the host gold's, bit for bit (a difference ends the run); then `--rounds`
(>= 5) rounds over the arms; per arm the median, min and max.  One process; run it under `timeout`:

  timeout -k 10 900 python tools/ilu0_bench.py --matrix synth:grid-2048 --out profiles/ilu0_grid2048.json
  timeout -k 10 900 python tools/ilu0_bench.py --matrix synth:grid-2048 --color --out profiles/ilu0_grid2048_colored.json
  timeout -k 10 600 python tools/ilu0_bench.py --matrix synth:rmat-14 --symmetrise --out profiles/ilu0_rmat14.json
  timeout -k 10 600 python tools/ilu0_bench.py --matrix synth:scircuit --out profiles/ilu0_scircuit.json

The sweep of the tier threshold: `make -C sparseharness_amd/csrc ilu0-lane LANE_WORK=<n>` builds
sparseharness_amd/variants/ilu0_lane<n>.so; run this tool once per build with SH_LIB=<that file> and --thin 256.

One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparseharness_amd import hostlib as H  # noqa: E402

from bfs_levels_bench import load_matrix, summary  # noqa: E402  (tools/ is the script's directory)
from trsv_bench import csr_from, pattern  # noqa: E402

SEED = 0x5EED


def full_system(n, r, c, grid):
    """The off-diagonal entries with the value -1 and a dominant diagonal."""
    diag = np.full(n, 4.0) if grid else 1.0 + np.bincount(r, minlength=n)
    rows = np.concatenate([r, np.arange(n)])
    return csr_from(n, rows, np.concatenate([c, np.arange(n)]), np.concatenate([-np.ones(len(r)), diag]))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--symmetrise", action="store_true")
    ap.add_argument("--color", action="store_true", help="permute by sh_color's classes first")
    ap.add_argument("--thin", default="0,64,256,1024,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-only", action="store_true", help="the host gold's work and time alone: no device")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    thins = [int(t) for t in args.thin.split(",")]
    n, rp, ci, va = load_matrix(args.matrix)
    r, c = pattern(n, rp, ci, args.symmetrise)
    grid = args.matrix.startswith("synth:grid-")
    res = {"tool": "tools/ilu0_bench.py", "matrix": args.matrix, "symmetrise": args.symmetrise, "color": args.color, "rows": n,
           "rounds": args.rounds, "lib": os.path.basename(os.environ.get("SH_LIB") or "libsparseharness_hip.so"),
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round"}
    if args.host_only:
        if args.color:
            raise SystemExit("--color needs the device")
        frp, fci, fva = full_system(n, r, c, grid)
        t0 = time.perf_counter()
        fig = H.ilu0_factor(frp, fci, fva, 0)[2]
        res.update({"nnz": len(fci), "gold_first_call_s": round(time.perf_counter() - t0, 4), **fig})
        print(json.dumps(res))
        return
    from sparseharness_amd.engine import Engine
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        if args.color:
            crp, cci, cva = csr_from(n, r, c, np.ones(len(r)))
            CG, cv = eng.color_graph(crp, cci, cva), eng.alloc(n)
            res["colors"] = eng.greedy_colors(CG, cv)[0]
            perm = np.argsort(cv.download(np.int32, n), kind="stable")
            pos = np.empty(n, np.int64)
            pos[perm] = np.arange(n)
            r, c = pos[r], pos[c]
            cv.free()
            CG.free()
        frp, fci, fva = full_system(n, r, c, grid)
        nnz = len(fci)
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.ilu0_graph(frp, fci)
        eng.synchronize()
        res.update({"nnz": nnz, "ilu0_graph_create_s": round(time.perf_counter() - t0, 4), "ilu0_graph_footprint_bytes": G.footprint,
                    "entries": G.entries, "levels": G.levels, "max_list": G.max_list, "max_width": G.max_width, "work": G.work})
        print(f"work = {G.work} look-ups ({G.entries} slots, {G.levels} levels, longest row {G.max_list})", file=sys.stderr, flush=True)
        vv, lv = eng.vector(fva.view(np.uint32)), eng.alloc(2 * nnz)

        def run(thin):
            eng.synchronize()
            t = time.perf_counter()
            out = eng.ilu0(G, vv, lv, 0, thin)
            return out, (time.perf_counter() - t) * 1e6

        t0 = time.perf_counter()
        gold = H.ilu0_factor(frp, fci, fva, 0)
        first_gold = time.perf_counter() - t0
        if any(gold[2][k] != getattr(G, k) for k in ("entries", "levels", "work", "max_list", "max_width")):
            raise SystemExit("the handle's figures differ from ilu0_factor's")
        plans = {}
        for thin in thins:   # warm-up and check, before anything is timed
            out, _ = run(thin)
            plans[thin] = out[:3]
            if not same_bits(lv.download(np.uint32, 2 * nnz).view(np.float64), gold[0]):
                raise SystemExit(f"lu differs from ilu0_factor's (thin = {thin})")
            if out[3:5] != (gold[2]["zero_pivots"], gold[2]["first_zero"]):
                raise SystemExit(f"the zero pivots differ from ilu0_factor's (thin = {thin})")
        dev, wall, gold_wall = {t: [] for t in thins}, {t: [] for t in thins}, []
        for _ in range(args.rounds):
            for thin in thins:
                out, w = run(thin)
                dev[thin].append(out[5])
                wall[thin].append(w)
            t0 = time.perf_counter()
            H.ilu0_factor(frp, fci, fva, 0)
            gold_wall.append((time.perf_counter() - t0) * 1e6)
        res["gold_wall_us"] = summary(gold_wall, 1.0)
        res["gold_first_call_s"] = round(first_gold, 4)
        res["arms"] = {}
        for thin in thins:
            d = summary(dev[thin], 1e3)
            res["arms"][f"thin={thin}"] = {"launches": plans[thin][0], "runs": plans[thin][1], "levels_in_runs": plans[thin][2],
                                           "device_us": d, "wall_us": summary(wall[thin], 1.0),
                                           "device_ratio_vs_gold_wall": round(d["median"] / res["gold_wall_us"]["median"], 5)}
        for h in (vv, lv, G):
            h.free()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        lines = [f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res.items() if k != "arms"]
        arms = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in res["arms"].items())
        with open(args.out, "w") as f:
            f.write("{\n" + ",\n".join(lines) + ",\n \"arms\": {\n" + arms + "\n }\n}\n")


if __name__ == "__main__":
    main()
