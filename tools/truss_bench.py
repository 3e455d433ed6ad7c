#!/usr/bin/env python3
"""What sh_truss costs, for one matrix, in one process and with the arms alternating:

  sh_truss          total device time of the call (the support pass and every round), the rounds, the levels, the sum of
                    min(deg u, deg v) over the edges walked, and the handle's build time and footprint;
  truss_numbers     wall time of the host's single-threaded bucket algorithm (hostlib.truss_numbers) -- the baseline.

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first: the handle and the host gold both ignore the direction.  synth:tgrid-<side> is the side x side grid
with one diagonal per cell (every inner edge in two triangles); the other generators are tools/bfs_levels_bench.py's.

Method: first truss, support, the ends of every edge, M, the triangles, max_truss and levels are compared with
truss_numbers' (a difference ends the run); then `--rounds` (>= 5) rounds over both arms; per arm the median, min and
max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/truss_bench.py --matrix synth:tgrid-2048 --out profiles/truss_tgrid2048.json
  timeout -k 10 600 python tools/truss_bench.py --matrix synth:rmat-16 --out profiles/truss_rmat16.json

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

GOLD, ARM = "truss_numbers", "sh_truss"


def triangulated_grid(side):
    """CSR arrays of the side x side grid with one diagonal per cell, every edge stored in both rows."""
    v = np.arange(side * side, dtype=np.int64).reshape(side, side)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel(), v[:-1, :-1].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel(), v[1:, 1:].ravel()])
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    order = np.lexsort((dst, src))
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=side * side))]).astype(np.int32)
    return rp, dst[order].astype(np.int32), np.ones(len(dst), np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:tgrid-2048")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    if args.matrix.startswith("synth:tgrid-"):
        rp, ci, va = triangulated_grid(int(args.matrix.split("-")[1]))
        n = len(rp) - 1
    else:
        n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va)
    t0 = time.perf_counter()
    want_eu, want_ev, want_sup, want_truss, m = H.truss_numbers(rp, ci, va)
    t_gold = time.perf_counter() - t0
    want = (int(want_truss.max()) if m else 0, len(np.unique(want_truss)), int(want_sup.sum()) // 3)
    res = {"tool": "tools/truss_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "edges": m, "triangles": want[2], "max_truss": want[0], "levels": want[1],
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.truss_graph(rp, ci, va)
        eng.synchronize()
        res.update({"truss_graph_create_s": round(time.perf_counter() - t0, 4), "truss_graph_footprint_bytes": G.footprint,
                    "max_degree": G.max_degree})
        vecs = [eng.alloc(max(m, 1)) for _ in range(4)]

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == GOLD:
                H.truss_numbers(rp, ci, va)
                r = None
            else:
                r = eng.truss_numbers(G, *vecs)
            return r, (time.perf_counter() - t) * 1e6

        for v in vecs:   # warm-up and check, before anything is timed
            v.fill(7, np.int32)
        r, _ = run(ARM)
        if G.edges != m or (r[0], r[1], r[4]) != want or not r[3]:
            raise SystemExit("sh_truss: M, max_truss, levels, triangles or complete differ from truss_numbers'")
        for v, w, name in zip(vecs, (want_truss, want_sup, want_eu, want_ev), ("truss", "support", "edge_u", "edge_v")):
            if not np.array_equal(v.download(np.int32, m), w):
                raise SystemExit(f"sh_truss: {name} differs from truss_numbers'")
        dev, wall, support_ns = [], {ARM: [], GOLD: []}, []
        for _ in range(args.rounds):
            for arm in (ARM, GOLD):
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev.append(r[9])
                    support_ns.append(r[9] - int(r[8].sum()))
                    last = r
        gold = summary(wall[GOLD], 1.0)
        res["arms"][GOLD] = {"wall_us": gold, "first_call_s": round(t_gold, 4)}
        rec = {"device_us": summary(dev, 1e3), "wall_us": summary(wall[ARM], 1.0), "support_pass_us": summary(support_ns, 1e3),
               "peel_rounds": last[2], "walked": int(last[7].sum())}
        rec["device_ratio_vs_truss_numbers_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
        res["arms"][ARM] = rec
        for h in vecs + [G]:
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
