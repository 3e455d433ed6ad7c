#!/usr/bin/env python3
"""What sh_msf costs, for one matrix, in one process and with the arms alternating:

  sh_msf       total device time of the call (start, all rounds, labels), the rounds, what every round walked, kept and
               hooked, and the handle's build time and footprint;
  msf_edges    wall time of the host's single-threaded Kruskal (clean, sort by KEY, union-find: hostlib.msf_edges) -- the
               baseline;
  sh_wcc       device time of the components alone on the same arrays (informational: what the forest costs beyond them).

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first.  --weights drawn: every stored entry gets a float32 from a seeded generator in [0, 1) (a drawn 0.0
would be no edge and becomes 2^-25), so the two directions of an edge differ and the smaller wins; --weights unit: every
weight is 1.0, so ties go by edge id and the first round builds long chains.

Method: first in_msf, comp, the ends and weights of every edge, M and the components are compared with msf_edges' (==; a
difference ends the run) and comp with sh_wcc's; then `--rounds` (>= 5) rounds over all arms; per arm the median, min and
max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/msf_bench.py --matrix synth:grid-2048 --out profiles/msf_grid2048.json
  timeout -k 10 600 python tools/msf_bench.py --matrix synth:rmat-18 --out profiles/msf_rmat18.json
  timeout -k 10 600 python tools/msf_bench.py --matrix synth:grid-2048 --weights unit --out profiles/msf_grid2048_unit.json

synth:star-<k> (this tool's own) is a hub with k leaves: every edge wants one best word.

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
ARMS = ("sh_msf", "msf_edges", "sh_wcc")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:grid-2048")
    ap.add_argument("--weights", choices=("drawn", "unit"), default="drawn")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    if args.matrix.startswith("synth:star-"):   # a hub (vertex 0) with k leaves, one entry per leaf: one best word for all
        k = int(args.matrix[len("synth:star-"):])
        n, rp, ci = k + 1, np.concatenate([[0], np.arange(k + 1)]).astype(np.int32), np.zeros(k, np.int32)
    else:
        n, rp, ci, _ = load_matrix(args.matrix)
    if args.weights == "drawn":
        va = np.random.default_rng(SEED).random(len(ci), dtype=np.float32)
        va[va == 0] = np.float32(2.0 ** -25)
    else:
        va = np.ones(len(ci), np.float32)
    t0 = time.perf_counter()
    eu, ev, weight, in_msf, comp, M, components = H.msf_edges(rp, ci, va)
    first = time.perf_counter() - t0
    res = {"tool": "tools/msf_bench.py", "matrix": args.matrix, "weights": args.weights, "rows": n, "entries": int(rp[-1]),
           "rounds": args.rounds, "seed": SEED,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.msf_graph(rp, ci, va)
        eng.synchronize()
        res.update({"msf_graph_create_s": round(time.perf_counter() - t0, 4), "msf_graph_footprint_bytes": G.footprint,
                    "edges": G.edges, "components": components, "tree_edges": n - components})
        WG = eng.wcc_graph(rp, ci, va)
        mv, uv, vv, wv = (eng.alloc(max(M, 1)) for _ in range(4))
        cv, kv = eng.alloc(max(n, 1)), eng.alloc(max(n, 1))

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == "sh_msf":
                r = eng.spanning_forest(G, mv, comp=cv)
            elif arm == "sh_wcc":
                r = eng.wcc(WG, kv)
            else:
                H.msf_edges(rp, ci, va)
                r = None
            return r, (time.perf_counter() - t) * 1e6

        # warm-up and check, before anything is timed
        for v in (mv, uv, vv, wv, cv, kv):
            v.fill(7, np.int32)
        r = eng.spanning_forest(G, mv, comp=cv, edge_u=uv, edge_v=vv, weight=wv)
        if G.edges != M or (r[0], r[1], r[3]) != (n - components, components, True):
            raise SystemExit("M, tree_edges, components or complete differ from msf_edges'")
        for name, v, k, ref in (("in_msf", mv, M, in_msf), ("edge_u", uv, M, eu), ("edge_v", vv, M, ev),
                                ("weight", wv, M, weight.view(np.int32)), ("comp", cv, n, comp)):
            if k and not np.array_equal(v.download(np.int32, k), ref):
                raise SystemExit(f"{name} differs from msf_edges'")
        run("sh_wcc")
        if n and not np.array_equal(kv.download(np.int32, n), comp):
            raise SystemExit("comp differs from sh_wcc's")
        dev, wall, last = {a: [] for a in ARMS}, {a: [] for a in ARMS}, {}
        for _ in range(args.rounds):
            for arm in ARMS:
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev[arm].append(r[-1])
                    last[arm] = r
        gold = summary(wall["msf_edges"], 1.0)
        res["arms"]["msf_edges"] = {"wall_us": gold, "first_call_s": round(first, 4)}
        r = last["sh_msf"]
        rec = {"device_us": summary(dev["sh_msf"], 1e3), "wall_us": summary(wall["sh_msf"], 1.0), "boruvka_rounds": r[2],
               "walked_per_round": r[4].tolist(), "kept_per_round": r[5].tolist(), "hooks_per_round": r[6].tolist(),
               "jumps_per_round": r[7].tolist(), "round_us": [round(x / 1e3, 1) for x in r[8].tolist()],
               "edges_walked": int(r[4].sum())}
        rec["device_ratio_vs_msf_edges_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
        res["arms"]["sh_msf"] = rec
        r = last["sh_wcc"]
        res["arms"]["sh_wcc"] = {"device_us": summary(dev["sh_wcc"], 1e3), "wall_us": summary(wall["sh_wcc"], 1.0), "wcc_rounds": r[2]}
        for h in (mv, uv, vv, wv, cv, kv, G, WG):
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
