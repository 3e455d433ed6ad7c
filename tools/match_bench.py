#!/usr/bin/env python3
"""What sh_match costs, for one matrix, in one process and with the arms alternating:

  sh_match h<heavy> s<seed>   total device time of the call (start and all rounds) under heavy 0 / 1 and seed 0 / 1, the
                              rounds, what every round walked, kept and matched, the handle's build time and footprint;
  greedy_matching h<heavy> s<seed>   wall time of the host's single-threaded definition in the same order (clean, sort
                              by MKEY, take: hostlib.greedy_matching) -- the baseline.

The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first.  --weights drawn: every stored entry gets a float32 from a seeded generator in [0, 1) (a drawn 0.0
would be no edge and becomes 2^-25), so the two directions of an edge differ and the smaller wins; --weights unit: every
weight is 1.0, so the low word of MKEY alone orders the edges: by edge id for seed 0 (one pair per round in places),
by mix32(e ^ 1) for seed 1.  --skip h0s0,h1s0 leaves arms out (a run of thousands of rounds is measured once, not five
times: --once h0s0 times an arm in one round only).

Method: first mate, in_match, the ends and weights of every edge, M and the pairs of every arm are compared with the
host gold's (==; a difference ends the run); then `--rounds` (>= 5) rounds over all arms; per arm the median, min and
max.  One process; run it under `timeout`:

  timeout -k 10 600 python tools/match_bench.py --matrix synth:grid-2048 --out profiles/match_grid2048.json
  timeout -k 10 600 python tools/match_bench.py --matrix synth:grid-2048 --weights unit --once h0s0,h1s0 --out profiles/match_grid2048_unit.json
  timeout -k 10 600 python tools/match_bench.py --matrix synth:rmat-18 --out profiles/match_rmat18.json
  timeout -k 10 600 python tools/match_bench.py --matrix synth:star-70001 --out profiles/match_star70001.json

synth:star-<k> (msf_bench.py's) is a hub with k leaves: every edge wants one best word.

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
ORDERS = [(0, 0), (0, 1), (1, 0), (1, 1)]
ROUND_CAP = 1 << 16   # the per-round arrays of a call have this many places at most (a run that needs more ends the tool)


def tag(order):
    return "h%ds%d" % order


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:grid-2048")
    ap.add_argument("--weights", choices=("drawn", "unit"), default="drawn")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip", default="", help="orders left out, as h<heavy>s<seed>, comma-separated")
    ap.add_argument("--once", default="", help="orders timed in the first round only")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    skip, once = set(filter(None, args.skip.split(","))), set(filter(None, args.once.split(",")))
    orders = [o for o in ORDERS if tag(o) not in skip]
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
    res = {"tool": "tools/match_bench.py", "matrix": args.matrix, "weights": args.weights, "rows": n, "entries": int(rp[-1]),
           "rounds": args.rounds, "seed": SEED, "timed_once": sorted(once), "skipped": sorted(skip),
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.match_graph(rp, ci, va)
        eng.synchronize()
        M = G.edges
        MAX_ROUNDS = min(n // 2 + 1, ROUND_CAP)
        res.update({"match_graph_create_s": round(time.perf_counter() - t0, 4), "match_graph_footprint_bytes": G.footprint,
                    "edges": M})
        tv = eng.alloc(max(n, 1))
        iv, uv, vv, wv = (eng.alloc(max(M, 1)) for _ in range(4))

        def run(arm, order):
            eng.synchronize()
            t = time.perf_counter()
            if arm == "sh_match":
                r = eng.matching(G, tv, heavy=order[0], seed=order[1], in_match=iv, max_rounds=MAX_ROUNDS)
            else:
                r = H.greedy_matching(rp, ci, va, heavy=order[0], seed=order[1])
            return r, (time.perf_counter() - t) * 1e6

        # warm-up and check, before anything is timed (the arms of --once: this call is their one timed run)
        dev, wall, gold_wall, last, first_gold = ({o: [] for o in orders} for _ in range(5))
        for o in orders:
            for v in (tv, iv, uv, vv, wv):
                v.fill(7, np.int32)
            t0 = time.perf_counter()
            eu, ev, weight, in_match, mate, gM, pairs = H.greedy_matching(rp, ci, va, heavy=o[0], seed=o[1])
            first_gold[o] = time.perf_counter() - t0
            eng.synchronize()
            t0 = time.perf_counter()
            r = eng.matching(G, tv, heavy=o[0], seed=o[1], in_match=iv, edge_u=uv, edge_v=vv, weight=wv, max_rounds=MAX_ROUNDS)
            w = (time.perf_counter() - t0) * 1e6
            if M != gM or (r[0], r[2]) != (pairs, True):
                raise SystemExit(f"{tag(o)}: M, pairs or complete differ from greedy_matching's")
            for name, v, k, ref in (("mate", tv, n, mate), ("in_match", iv, M, in_match), ("edge_u", uv, M, eu),
                                    ("edge_v", vv, M, ev), ("weight", wv, M, weight.view(np.int32))):
                if k and not np.array_equal(v.download(np.int32, k), ref):
                    raise SystemExit(f"{tag(o)}: {name} differs from greedy_matching's")
            last[o] = r
            if tag(o) in once:
                dev[o].append(r[-1])
                wall[o].append(w)
                gold_wall[o].append(first_gold[o] * 1e6)
        for _ in range(args.rounds):
            for o in orders:
                if tag(o) in once:
                    continue
                r, w = run("sh_match", o)
                dev[o].append(r[-1])
                wall[o].append(w)
                last[o] = r
                _, w = run("greedy_matching", o)
                gold_wall[o].append(w)
        for o in orders:
            r = last[o]
            gold = summary(gold_wall[o], 1.0)
            rec = {"device_us": summary(dev[o], 1e3), "wall_us": summary(wall[o], 1.0), "gold_wall_us": gold,
                   "gold_first_call_s": round(first_gold[o], 4), "samples": len(dev[o]), "pairs": r[0], "match_rounds": r[1],
                   "edges_walked": int(r[3].sum()), "edges_kept": int(r[4].sum())}
            if r[1] <= 64:
                rec.update({"walked_per_round": r[3].tolist(), "kept_per_round": r[4].tolist(),
                            "matched_per_round": r[5].tolist(), "round_us": [round(x / 1e3, 1) for x in r[6].tolist()]})
            else:
                rec.update({"walked_first_rounds": r[3][:8].tolist(), "matched_first_rounds": r[5][:8].tolist(),
                            "rounds_matching_one_pair": int((r[5] == 1).sum()),
                            "round_us_median": round(float(np.median(r[6])) / 1e3, 1)})
            rec["device_ratio_vs_gold_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
            res["arms"][tag(o)] = rec
        for h in (tv, iv, uv, vv, wv, G):
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
