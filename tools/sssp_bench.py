#!/usr/bin/env python3
"""What a bucketed SSSP costs next to the (min,+) iteration loops: for one matrix and a few sources, in the same
process and alternating:

  sh_iterate            SH_MIN_PLUS_F32, alpha = beta = 0, y0 = x0, under the plan sh_csr_upload chooses by default, with a
                        delta so small (1e-30) that it stops only when nothing changes;
  sh_iterate_frontier   the same at its default dense_share;
  sh_sssp               at the default bucket width, at +Inf (one bucket) and at every `--factors` multiple of the default
                        -- the first two also with the predecessor pass.

Sources: vertex 0 as the apps, plus `--sources` seeded random vertices with non-empty out-lists.

Method: one warm-up of every arm, in which every arm's dist is compared bitwise with sh_iterate's; then `--rounds` (>= 5)
rounds over all arms; per arm the median, min and max of the total device time (total_ns of the C ABI) and the median
wall time of the call.

  python tools/sssp_bench.py --matrix synth:grid-2048 --out profiles/sssp_grid2048.json
  python tools/sssp_bench.py --matrix synth:scircuit --out profiles/sssp_scircuit.json
  python tools/sssp_bench.py --matrix synth:rmat-23 --out profiles/sssp_rmat23.json
  python tools/sssp_bench.py --matrix synth:powerlaw-10000000-200000000 --out profiles/sssp_powerlaw.json

One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparseharness_amd.engine import MIN_PLUS_F32, Engine  # noqa: E402

from bfs_levels_bench import dump, load_matrix, summary  # noqa: E402  (tools/ is the script's directory)

FLT_MAX = np.float32(3.4028235e38)
EXACT = 1e-30   # sh_iterate's delta: below every float32 difference, so the loop stops at the exact fixed point


def arm_name(arm):
    what, with_pred = arm
    name = "default" if what == -1.0 else "one bucket" if what == float("inf") else f"delta={what:g}"
    return name + (" +pred" if with_pred else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--factors", default="0.0625,0.25,0.5,2,4,16", help="multiples of the default bucket width, comma-separated")
    ap.add_argument("--sources", type=int, default=2, help="seeded random sources with non-empty out-lists besides vertex 0")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=1 << 20)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    vals = np.ascontiguousarray(va, np.float32)
    inb = (ci >= 0) & (ci < n) & np.isfinite(vals)
    outdeg = np.bincount(ci[inb], minlength=n)
    rng = np.random.default_rng(23)
    cand = np.flatnonzero(outdeg > 0)
    sources = [0] + [int(v) for v in rng.choice(cand, min(args.sources, len(cand)), replace=False)]
    res = {"tool": "tools/sssp_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "timing": "device_us: total_ns of the C ABI (events around every round / launch, the set-up launch and the predecessor "
                     "pass); wall_us_median: the call as the host sees it; median / min / max over the rounds, arms alternating "
                     "inside a round", "sources": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        A = eng.upload_csr(n, n, rp, ci, vals)   # what sh_csr_upload chooses (the environment included)
        eng.synchronize()
        t_up = time.perf_counter() - t0
        F = eng.frontier(A, rp, ci, vals)
        t0 = time.perf_counter()
        G = eng.sssp_graph(rp, ci, vals)
        eng.synchronize()
        t_g = time.perf_counter() - t0
        default = G.delta
        res.update({"plan": A.describe(), "upload_s": round(t_up, 4), "matrix_footprint_bytes": A.footprint(),
                    "sssp_graph_create_s": round(t_g, 4), "sssp_graph_footprint_bytes": G.footprint, "edges": G.edges,
                    "default_delta": default})
        widths = [-1.0, float("inf")] + [default * float(f) for f in args.factors.split(",") if f]
        xv, yv, sc, dv, pv = eng.alloc(n), eng.alloc(n), eng.alloc(n), eng.alloc(n), eng.alloc(n)
        for source in sources:
            x0 = np.full(n, FLT_MAX, np.float32)
            x0[source] = 0.0

            def run(arm):
                xv.upload(x0)
                yv.upload(x0)
                eng.synchronize()
                t = time.perf_counter()
                if arm == "sh_iterate":
                    it, cv, per, total = eng.iterate(MIN_PLUS_F32, A, xv, yv, sc, 0.0, 0.0, delta=EXACT, max_iters=args.max_iters)
                    r = (it, total, cv)
                elif arm == "sh_iterate_frontier":
                    r = eng.iterate_frontier(MIN_PLUS_F32, A, F, xv, yv, sc, 0.0, 0.0, delta=EXACT, max_iters=args.max_iters)
                    r = (r[0], r[6], r[1])
                else:
                    r = eng.sssp(G, xv, dv, pv if arm[1] else None, delta=arm[0], max_rounds=args.max_rounds)
                return r, (time.perf_counter() - t) * 1e6

            # (the predecessor pass costs the same under every width: it is timed with the default and with one bucket only)
            arms = ["sh_iterate", "sh_iterate_frontier"] + [(w, p) for w in widths for p in (False, True) if not p or w in widths[:2]]
            (b_it, _, b_cv), _ = run("sh_iterate")
            if not b_cv:
                raise SystemExit(f"source {source}: sh_iterate did not reach its fixed point in {args.max_iters} launches")
            want = xv.download(np.uint32)
            for arm in arms[1:]:   # warm-up and check
                r, _ = run(arm)
                got = (xv if arm == "sh_iterate_frontier" else dv).download(np.uint32)
                if not np.array_equal(got, want) or (not isinstance(arm, str) and not r[3]):
                    raise SystemExit(f"source {source}, {arm}: dist differs from sh_iterate's")
            dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
            for _ in range(args.rounds):
                for arm in arms:
                    r, w = run(arm)
                    dev[arm].append(r[1] if isinstance(arm, str) else r[8])
                    wall[arm].append(w)
                    last[arm] = r
            out = {"out_list_length": int(outdeg[source]), "launches_of_sh_iterate": b_it, "arms": {}}
            for arm in arms:
                rec = {"device_us": summary(dev[arm], 1e3), "wall_us_median": round(statistics.median(wall[arm]), 1)}
                if not isinstance(arm, str):
                    rounds, buckets, reached, complete, relaxed, sizes, edges, per, total = last[arm]
                    rec.update({"rounds": rounds, "buckets": buckets, "reached": reached, "edges_looked_at": relaxed,
                                "edges_looked_at_per_edge": round(relaxed / max(G.edges, 1), 3),
                                "us_per_round": round(float(per.sum()) / 1e3 / max(rounds, 1), 3),
                                "largest_round": int(sizes.max()) if rounds else 0,
                                "us_outside_the_rounds": round((total - float(per.sum())) / 1e3, 3)})
                out["arms"][arm if isinstance(arm, str) else arm_name(arm)] = rec
            base = out["arms"]["sh_iterate"]["device_us"]["median"]
            fr = out["arms"]["sh_iterate_frontier"]["device_us"]["median"]
            for rec in out["arms"].values():
                rec["device_ratio_vs_sh_iterate"] = round(rec["device_us"]["median"] / base, 4)
                rec["device_ratio_vs_sh_iterate_frontier"] = round(rec["device_us"]["median"] / fr, 4)
            # the widths of the sweep are kept short: [factor of the default, device_us median, min, max, ratio to sh_iterate, rounds, buckets, edges looked at]
            out["sweep"] = {}
            for w in widths[2:]:
                rec = out["arms"].pop(arm_name((w, False)))
                out["sweep"][arm_name((w, False))] = [round(w / default, 4) if default else None, rec["device_us"]["median"],
                                                      rec["device_us"]["min"], rec["device_us"]["max"], rec["device_ratio_vs_sh_iterate"],
                                                      rec["rounds"], rec["buckets"], rec["edges_looked_at"]]
            res["sources"][str(source)] = out
            print(f"source {source}: " + json.dumps({**{k: (v["device_us"]["median"], v["device_ratio_vs_sh_iterate"])
                                                        for k, v in out["arms"].items()},
                                                     **{k: (v[1], v[4]) for k, v in out["sweep"].items()}}), file=sys.stderr, flush=True)
        # the sweep's verdict: per width the worst ratio to sh_iterate over the sources (without the predecessor pass)
        worst = {}
        for w in widths:
            k = arm_name((w, False))
            worst[k] = max(s["arms"][k]["device_ratio_vs_sh_iterate"] if w in widths[:2] else s["sweep"][k][4]
                           for s in res["sources"].values())
        res["worst_ratio_vs_sh_iterate_per_width"] = worst
        for h in (xv, yv, sc, dv, pv, G, F, A):
            h.free()
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(dump(res))


if __name__ == "__main__":
    main()
