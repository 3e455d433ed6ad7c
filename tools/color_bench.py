#!/usr/bin/env python3
"""What sh_color costs, for one matrix, in one process and with the arms alternating:

  sh_color order=o    o in {0 natural, 1 random, 2 largest degree first}: total device time of the call, the rounds, the
                      colours, the list entries looked at, and the handle's build time and footprint;
  greedy_colors o     wall time of the host's single-threaded first-fit loop in the same order (hostlib.greedy_colors) --
                      the baseline.

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first: the handle and the host gold both ignore the direction.  Beside the colours the file holds
max_degree + 1, the bound of every greedy colouring, and degeneracy + 1 (from sh_core on the same matrix), the bound of
the smallest-last order.

Method: first every order's colours, number of colours, rounds and round sizes are compared with greedy_colors' (==; a
difference ends the run); then `--rounds` (>= 5) rounds over all arms; per arm the median, min and max.  One process; run
it under `timeout`:

  timeout -k 10 600 python tools/color_bench.py --matrix synth:grid-2048 --out profiles/color_grid2048.json
  timeout -k 10 600 python tools/color_bench.py --matrix synth:rmat-18 --out profiles/color_rmat18.json

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

ORDERS = (0, 1, 2)
SEED = 0x5EED


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:grid-2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va)
    want, first = {}, {}
    for o in ORDERS:
        t0 = time.perf_counter()
        want[o] = H.greedy_colors(rp, ci, va, order=o, seed=SEED)
        first[o] = time.perf_counter() - t0
    res = {"tool": "tools/color_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "seed": SEED,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.color_graph(rp, ci, va)
        eng.synchronize()
        res.update({"color_graph_create_s": round(time.perf_counter() - t0, 4), "color_graph_footprint_bytes": G.footprint,
                    "edges": G.edges, "max_degree": G.max_degree, "max_degree_plus_1": G.max_degree + 1})
        cv = eng.alloc(n)
        CG = eng.core_graph(rp, ci, va)   # degeneracy + 1 bounds the colours of the smallest-last order
        res["degeneracy_plus_1"] = eng.core_numbers(CG, cv)[0] + 1
        CG.free()
        arms = [f"sh_color order={o}" for o in ORDERS] + [f"greedy_colors order={o}" for o in ORDERS]

        def run(arm):
            o = int(arm.split("=")[1])
            eng.synchronize()
            t = time.perf_counter()
            if arm.startswith("sh_color"):
                r = eng.greedy_colors(G, cv, order=o, seed=SEED)
            else:
                H.greedy_colors(rp, ci, va, order=o, seed=SEED)
                r = None
            return r, (time.perf_counter() - t) * 1e6

        for o in ORDERS:   # warm-up and check, before anything is timed
            cv.fill(7, np.int32)
            r, _ = run(f"sh_color order={o}")
            color, colors, depth = want[o]
            if (r[0], r[1], r[2], r[3]) != (colors, int(depth.max()) + 1 if n else 0, True, n):
                raise SystemExit(f"order {o}: colors, rounds, complete or coloured differ from greedy_colors'")
            if not np.array_equal(cv.download(np.int32, n), color):
                raise SystemExit(f"order {o}: the colours differ from greedy_colors'")
            if not np.array_equal(r[4], np.bincount(depth, minlength=r[1])):
                raise SystemExit(f"order {o}: the round sizes differ from the histogram of greedy_colors' depths")
        dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for arm in arms:
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev[arm].append(r[7])
                    last[arm] = r
        for o in ORDERS:
            gold = summary(wall[f"greedy_colors order={o}"], 1.0)
            res["arms"][f"greedy_colors order={o}"] = {"wall_us": gold, "first_call_s": round(first[o], 4)}
            r = last[f"sh_color order={o}"]
            rec = {"device_us": summary(dev[f"sh_color order={o}"], 1e3), "wall_us": summary(wall[f"sh_color order={o}"], 1.0),
                   "colors": r[0], "jp_rounds": r[1], "largest_round": int(r[4].max()) if r[1] else 0,
                   "edges_looked_at": int(r[5].sum())}
            rec["device_ratio_vs_greedy_colors_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
            res["arms"][f"sh_color order={o}"] = rec
        for h in [cv, G]:
            h.free()
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in res.items() if k != "arms") + ',\n "arms": {\n'
                    + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in res["arms"].items()) + "\n }\n}\n")


if __name__ == "__main__":
    main()
