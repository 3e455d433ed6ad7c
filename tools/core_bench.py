#!/usr/bin/env python3
"""What sh_core costs, for one matrix, in one process and with the arms alternating:

  sh_core chase=c   c in {0, 4, 16, 64}: total device time of the call, the rounds, the vertices taken from work lists and
                    those chased, the list entries looked at, and the handle's build time and footprint;
  core_numbers      wall time of the host's single-threaded bucket algorithm (hostlib.core_numbers) -- the baseline.

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first: the handle and the host gold both ignore the direction.

Method: first every arm's core, deg, degeneracy and levels are compared with core_numbers' (a difference ends the run);
then `--rounds` (>= 5) rounds over all arms; per arm the median, min and max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/core_bench.py --matrix synth:grid-2048 --out profiles/core_grid2048.json
  timeout -k 10 600 python tools/core_bench.py --matrix synth:rmat-18 --out profiles/core_rmat18.json

The binding's default `chase` is read off these two files: the fastest arm on the 2048 x 2048 grid, provided it is no
slower than chase = 0 on R-MAT-18 by more than the spread (min to max) of the rounds there.

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

GOLD = "core_numbers"
CHASES = (0, 4, 16, 64)


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
    t0 = time.perf_counter()
    want_core, want_deg, want_edges = H.core_numbers(rp, ci, va)
    t_gold = time.perf_counter() - t0
    want = (int(want_core.max()) if n else 0, len(np.unique(want_core)))
    res = {"tool": "tools/core_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "edges": want_edges, "degeneracy": want[0], "levels": want[1], "max_degree": int(want_deg.max()) if n else 0,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.core_graph(rp, ci, va)
        eng.synchronize()
        res.update({"core_graph_create_s": round(time.perf_counter() - t0, 4), "core_graph_footprint_bytes": G.footprint})
        cv, dv = eng.alloc(n), eng.alloc(n)
        arms = [f"sh_core chase={c}" for c in CHASES] + [GOLD]

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == GOLD:
                H.core_numbers(rp, ci, va)
                r = None
            else:
                r = eng.core_numbers(G, cv, dv, chase=int(arm.split("=")[1]))
            return r, (time.perf_counter() - t) * 1e6

        for arm in arms[:-1]:   # warm-up and check, before anything is timed
            cv.fill(7, np.int32)
            r, _ = run(arm)
            if (r[0], r[1]) != want or not r[3]:
                raise SystemExit(f"{arm}: degeneracy, levels or complete differ from core_numbers'")
            if not np.array_equal(cv.download(np.int32, n), want_core) or not np.array_equal(dv.download(np.int32, n), want_deg):
                raise SystemExit(f"{arm}: core or deg differs from core_numbers'")
        dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for arm in arms:
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev[arm].append(r[9])
                    last[arm] = r
        gold = summary(wall[GOLD], 1.0)
        res["arms"][GOLD] = {"wall_us": gold, "first_call_s": round(t_gold, 4)}
        for arm in arms[:-1]:
            r = last[arm]
            rec = {"device_us": summary(dev[arm], 1e3), "wall_us": summary(wall[arm], 1.0), "peel_rounds": r[2],
                   "listed": int(r[5].sum()), "chased": int(r[6].sum()), "edges_looked_at": int(r[7].sum())}
            rec["device_ratio_vs_core_numbers_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
            res["arms"][arm] = rec
        base = res["arms"]["sh_core chase=0"]["device_us"]
        res["chase0_spread_us"] = round(base["max"] - base["min"], 3)
        for c in CHASES[1:]:
            res[f"chase{c}_vs_chase0"] = round(res["arms"][f"sh_core chase={c}"]["device_us"]["median"] / max(base["median"], 1e-9), 4)
        for h in [cv, dv, G]:
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
