#!/usr/bin/env python3
"""What sh_tri costs, for one matrix, in one process and with the arms alternating:

  sh_tri order=o tri=yes|no   o in {0, 1}: total device time of the call with and without the per-vertex counts, the
                              triangles, the probes, the longest forward list, the handle's build time and footprint;
  triangle_counts             wall time of the host's single-threaded forward algorithm (hostlib.triangle_counts) -- the
                              baseline.

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first: the handle and the host gold both ignore the direction.

Method: first every arm's tri, deg and total are compared with triangle_counts' (a difference ends the run); then
`--rounds` (>= 5) rounds over all arms; per arm the median, min and max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/tri_bench.py --matrix synth:scircuit --out profiles/tri_scircuit.json
  timeout -k 10 600 python tools/tri_bench.py --matrix synth:rmat-18 --out profiles/tri_rmat18.json
  timeout -k 10 600 python tools/tri_bench.py --matrix synth:grid-2048 --out profiles/tri_grid2048.json

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

GOLD = "triangle_counts"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va)
    t0 = time.perf_counter()
    want_tri, want_deg = H.triangle_counts(rp, ci, va)
    t_gold = time.perf_counter() - t0
    want_total = int(want_tri.sum()) // 3
    res = {"tool": "tools/tri_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "triangles": want_total, "max_degree": int(want_deg.max()) if n else 0,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        graphs = {}
        for order in (0, 1):
            eng.synchronize()
            t0 = time.perf_counter()
            graphs[order] = eng.tri_graph(rp, ci, va, order=order)
            eng.synchronize()
            res[f"order{order}"] = {"tri_graph_create_s": round(time.perf_counter() - t0, 4), "max_forward": graphs[order].max_forward}
        res.update({"edges": graphs[1].edges, "tri_graph_footprint_bytes": graphs[1].footprint})
        tv, dv = eng.alloc(2 * n), eng.alloc(n)
        arms = [f"sh_tri order={o} tri={t}" for o in (0, 1) for t in ("yes", "no")] + [GOLD]

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == GOLD:
                H.triangle_counts(rp, ci, va)
                r = None
            else:
                r = eng.triangles(graphs[int(arm.split("=")[1][0])], tv if arm.endswith("yes") else None, dv)
            return r, (time.perf_counter() - t) * 1e6

        for arm in arms[:-1]:   # warm-up and check, before anything is timed
            tv.fill(7, np.int32)
            r, _ = run(arm)
            if r[0] != want_total or not np.array_equal(dv.download(np.int32, n), want_deg):
                raise SystemExit(f"{arm}: the total or deg differs from triangle_counts'")
            if arm.endswith("yes") and not np.array_equal(tv.download(np.uint32, 2 * n).view(np.uint64), want_tri):
                raise SystemExit(f"{arm}: tri differs from triangle_counts'")
        dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for arm in arms:
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev[arm].append(r[2])
                    last[arm] = r
        gold = summary(wall[GOLD], 1.0)
        res["arms"][GOLD] = {"wall_us": gold, "first_call_s": round(t_gold, 4)}
        for arm in arms[:-1]:
            rec = {"device_us": summary(dev[arm], 1e3), "wall_us": summary(wall[arm], 1.0), "probes": last[arm][1]}
            rec["device_ratio_vs_triangle_counts_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
            res["arms"][arm] = rec
        for t in ("yes", "no"):
            a0, a1 = res["arms"][f"sh_tri order=0 tri={t}"], res["arms"][f"sh_tri order=1 tri={t}"]
            res[f"order1_vs_order0_tri_{t}"] = round(a1["device_us"]["median"] / max(a0["device_us"]["median"], 1e-9), 4)
        for h in [tv, dv, graphs[0], graphs[1]]:
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
