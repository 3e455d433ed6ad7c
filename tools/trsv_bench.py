#!/usr/bin/env python3
"""What sh_trsv costs, for one matrix, in one process and with the arms alternating:

  sh_trsv        device time of one float64 solve with the lower triangle of the matrix, for every `thin` of --thin
                 (consecutive levels of at most `thin` rows share a one-workgroup launch; 0: one launch per level), with
                 the launches, the runs and the levels those hold;
  trsv_solve     wall time of the host's serial substitution in the same summation order (hostlib.trsv_solve) -- the
                 baseline.

The matrix: the pattern of --matrix, symmetrised (--symmetrise) or as given, its strictly-lower entries with the value -1
and a diagonal of 1 + the entries of the row (diagonally dominant, so x stays bounded; synth:grid-<side>: 4, the 5-point
Laplacian).  --color permutes it first by sh_color's classes (stable by colour): rows of one colour share a level.

Method: first x of every arm is compared with the host gold's, bit for bit (a difference ends the run); then `--rounds`
(>= 5) rounds over the arms; per arm the median, min and max.  One process; run it under `timeout`:

  timeout -k 10 900 python tools/trsv_bench.py --matrix synth:grid-2048 --out profiles/trsv_grid2048.json
  timeout -k 10 900 python tools/trsv_bench.py --matrix synth:grid-2048 --color --out profiles/trsv_grid2048_colored.json
  timeout -k 10 600 python tools/trsv_bench.py --matrix synth:rmat-18 --symmetrise --out profiles/trsv_rmat18.json
  timeout -k 10 600 python tools/trsv_bench.py --matrix synth:scircuit --out profiles/trsv_scircuit.json

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


def csr_from(n, r, c, v):
    o = np.argsort(r, kind="stable")
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rp, c[o].astype(np.int32), v[o].astype(np.float32)


def pattern(n, rp, ci, symmetrise):
    """The off-diagonal pairs (r, c) of the pattern, once each, both ways when symmetrise."""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    c = ci.astype(np.int64)
    keep = (c >= 0) & (c < n) & (c != r)
    r, c = r[keep], c[keep]
    if symmetrise:
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
    key = np.unique(r * n + c)
    return key // n, key % n


def lower_system(n, r, c, grid):
    """The strictly-lower entries with the value -1 and a dominant diagonal."""
    low = c < r
    r, c = r[low], c[low]
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
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    thins = [int(t) for t in args.thin.split(",")]
    n, rp, ci, va = load_matrix(args.matrix)
    r, c = pattern(n, rp, ci, args.symmetrise)
    res = {"tool": "tools/trsv_bench.py", "matrix": args.matrix, "symmetrise": args.symmetrise, "color": args.color, "rows": n,
           "rounds": args.rounds, "seed": SEED,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round"}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        if args.color:
            frp, fci, fva = csr_from(n, r, c, np.ones(len(r)))
            CG, cv = eng.color_graph(frp, fci, fva), eng.alloc(n)
            res["colors"] = eng.greedy_colors(CG, cv)[0]
            perm = np.argsort(cv.download(np.int32, n), kind="stable")
            pos = np.empty(n, np.int64)
            pos[perm] = np.arange(n)
            r, c = pos[r], pos[c]
            cv.free()
            CG.free()
        lrp, lci, lva = lower_system(n, r, c, args.matrix.startswith("synth:grid-"))
        b = np.random.default_rng(SEED).normal(size=n)
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.trsv_graph(lrp, lci, lva)
        eng.synchronize()
        res.update({"trsv_graph_create_s": round(time.perf_counter() - t0, 4), "trsv_graph_footprint_bytes": G.footprint,
                    "entries": G.entries, "levels": G.levels, "max_list": G.max_list, "max_width": G.max_width})
        bv, xv = eng.vector(b.view(np.uint32)), eng.alloc(2 * n)

        def run(thin):
            eng.synchronize()
            t = time.perf_counter()
            out = eng.trsv(G, bv, xv, 0, thin)
            return out, (time.perf_counter() - t) * 1e6

        t0 = time.perf_counter()
        gold = H.trsv_solve(lrp, lci, lva, b)
        first_gold = time.perf_counter() - t0
        if gold[2]["levels"] != G.levels or gold[2]["entries"] != G.entries:
            raise SystemExit("levels or entries differ from trsv_solve's")
        plans = {}
        for thin in thins:   # warm-up and check, before anything is timed
            out, _ = run(thin)
            plans[thin] = out[:3]
            if not same_bits(xv.download(np.uint32, 2 * n).view(np.float64), gold[0]):
                raise SystemExit(f"x differs from trsv_solve's (thin = {thin})")
        dev, wall, gold_wall = {t: [] for t in thins}, {t: [] for t in thins}, []
        for _ in range(args.rounds):
            for thin in thins:
                out, w = run(thin)
                dev[thin].append(out[3])
                wall[thin].append(w)
            t0 = time.perf_counter()
            H.trsv_solve(lrp, lci, lva, b)
            gold_wall.append((time.perf_counter() - t0) * 1e6)
        res["gold_wall_us"] = summary(gold_wall, 1.0)
        res["gold_first_call_s"] = round(first_gold, 4)
        res["arms"] = {}
        for thin in thins:
            d = summary(dev[thin], 1e3)
            res["arms"][f"thin={thin}"] = {"launches": plans[thin][0], "runs": plans[thin][1], "levels_in_runs": plans[thin][2],
                                           "device_us": d, "wall_us": summary(wall[thin], 1.0),
                                           "device_ratio_vs_gold_wall": round(d["median"] / res["gold_wall_us"]["median"], 5)}
        for h in (bv, xv, G):
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
