#!/usr/bin/env python3
"""What sh_bc costs, for one matrix, in one process and with the arms alternating:

  sh_bc          total device time of one call from `--sources` drawn sources (both sweeps of every source), and per
                 source its depth, the largest path count and the out-list entries walked forward;
  bfs_levels     the device time of as many sh_bfs_levels calls from the same sources: the forward sweep's floor;
  bc_scores      wall time of the host's serial Brandes in the same summation order (hostlib.bc_scores) -- the baseline.

The sources are drawn by a seeded generator among the vertices with an out-edge; four per trial is the usual convention
for this kernel.  synth:grid-<side> above 1029 overflows sigma (C(n, n / 2) leaves float64 near n = 1030).

Method: first bc, sigma and level of the call are compared with the host gold's, bit for bit (a difference ends the run;
where sigma has overflowed a NaN must stand where a NaN stands); then `--rounds` (>= 5) rounds over the arms; per arm the
median, min and max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/bc_bench.py --matrix synth:rmat-18 --sources 4 --out profiles/bc_rmat18.json
  timeout -k 10 600 python tools/bc_bench.py --matrix synth:scircuit --sources 4 --out profiles/bc_scircuit.json
  timeout -k 10 600 python tools/bc_bench.py --matrix synth:grid-512 --sources 4 --out profiles/bc_grid512.json

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
from sparseharness_amd.engine import Engine  # noqa: E402

from bfs_levels_bench import load_matrix, summary  # noqa: E402  (tools/ is the script's directory)

SEED = 0x5EED


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    has_out = np.bincount(ci[(ci >= 0) & (ci < n)], minlength=n) > 0
    sources = np.random.default_rng(SEED).choice(np.nonzero(has_out)[0], args.sources, replace=False).astype(np.int32)
    res = {"tool": "tools/bc_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "seed": SEED, "sources": sources.tolist(),
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round"}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.bc_graph(rp, ci, va)
        eng.synchronize()
        res.update({"bc_graph_create_s": round(time.perf_counter() - t0, 4), "bc_graph_footprint_bytes": G.footprint,
                    "edges": G.edges, "max_list": G.max_list})
        B = eng.bfs_graph(rp, ci, va)
        bc, sg, lv, bl = eng.alloc(2 * n), eng.alloc(2 * n), eng.alloc(n), eng.alloc(n)
        x0 = []
        for s in sources:
            x = np.zeros(n, np.int32)
            x[s] = 1
            x0.append(eng.vector(x))

        def run_bc():
            eng.synchronize()
            t = time.perf_counter()
            r = eng.betweenness(G, sources, bc, 0, sg, lv)
            return r, (time.perf_counter() - t) * 1e6

        def run_bfs():
            eng.synchronize()
            t = time.perf_counter()
            ns = sum(eng.bfs_levels(B, x, bl)[-1] for x in x0)
            return ns, (time.perf_counter() - t) * 1e6

        # warm-up and check, before anything is timed
        t0 = time.perf_counter()
        gold = H.bc_scores(rp, ci, va, sources)
        first_gold = time.perf_counter() - t0
        r, _ = run_bc()
        run_bfs()
        got = (bc.download(np.uint32, 2 * n).view(np.float64), sg.download(np.uint32, 2 * n).view(np.float64))
        for name, a, b in (("bc", got[0], gold[0]), ("sigma", got[1], gold[1])):
            if not same_bits(a, b):
                raise SystemExit(f"{name} differs from bc_scores's")
        if not np.array_equal(lv.download(np.int32, n), gold[2]) or not np.array_equal(r[1], gold[3]) \
                or not np.array_equal(r[4], gold[6]) or not same_bits(r[3], gold[5]):
            raise SystemExit("level, depth, edges or sigma_max differ from bc_scores's")
        dev, wall, bfs_dev, bfs_wall, gold_wall = [], [], [], [], []
        for _ in range(args.rounds):
            r, w = run_bc()
            dev.append(r[-1])
            wall.append(w)
            ns, w = run_bfs()
            bfs_dev.append(ns)
            bfs_wall.append(w)
            t0 = time.perf_counter()
            H.bc_scores(rp, ci, va, sources)
            gold_wall.append((time.perf_counter() - t0) * 1e6)
        res.update({"steps": r[0], "depth_per_source": r[1].tolist(), "reached_per_source": r[2].tolist(),
                    "sigma_max_per_source": [float(x) for x in r[3]], "edges_per_source": r[4].tolist(),
                    "source_us": [round(x / 1e3, 1) for x in r[5].tolist()],
                    "device_us": summary(dev, 1e3), "wall_us": summary(wall, 1.0),
                    "bfs_levels_device_us": summary(bfs_dev, 1e3), "bfs_levels_wall_us": summary(bfs_wall, 1.0),
                    "gold_wall_us": summary(gold_wall, 1.0), "gold_first_call_s": round(first_gold, 4)})
        res["device_ratio_vs_gold_wall"] = round(res["device_us"]["median"] / res["gold_wall_us"]["median"], 5)
        res["device_ratio_vs_bfs_levels"] = round(res["device_us"]["median"] / res["bfs_levels_device_us"]["median"], 3)
        for h in [bc, sg, lv, bl, G, B] + x0:
            h.free()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res.items()) + "\n}\n")


if __name__ == "__main__":
    main()
