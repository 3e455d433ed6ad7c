#!/usr/bin/env python3
"""What a direction-optimising BFS with levels costs next to the (or,and) iteration loops: for one matrix and a few
sources, in the same process and alternating:

  sh_iterate            SH_OR_AND_I32, alpha = beta = 1, under the plan sh_csr_upload chooses by default (reachability only);
  sh_iterate_frontier   the same at its default dense_share;
  sh_bfs_levels         for every (up_share, down_share) of the sweep -- always including top-down only (1, 0), bottom-up
                        only (0, 0) and the engine's default (-1, -1), these three also with the parent pass.

Sources: vertex 0 as the apps, plus `--sources` seeded random vertices with non-empty out-lists (an R-MAT's vertex 0 is a
hub; a run from a leaf looks different).

Method: one warm-up of every arm (levels are compared between all pairs of the sweep, and (level >= 0) with sh_iterate's
final vector), then `--rounds` (>= 5) rounds over all arms; per arm the median, min and max of the total device time
(total_ns of the C ABI) and of the wall time of the call.  For the three fixed pairs also (for the default: the last run's per-level mode / size / edges / ns) the share of the graph's edges the
bottom-up steps looked at and the device time per step of each direction; for the other pairs of the sweep one short
record (device time, ratio to sh_iterate, steps by direction) and, over all sources, the worst ratio per pair.

  python tools/bfs_levels_bench.py --matrix synth:rmat-23 --out profiles/bfs_levels_rmat23.json
  python tools/bfs_levels_bench.py --matrix synth:grid-2048 --out profiles/bfs_levels_grid2048.json
  python tools/bfs_levels_bench.py --matrix synth:scircuit --out profiles/bfs_levels_scircuit.json
  python tools/bfs_levels_bench.py --matrix synth:powerlaw-10000000-200000000 --out profiles/bfs_levels_powerlaw.json

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
from sparseharness_amd import hostlib as H  # noqa: E402
from sparseharness_amd.engine import OR_AND_I32, Engine  # noqa: E402

from frontier_bench import grid_graph  # noqa: E402  (tools/ is the script's directory)

FIXED = [(1.0, 0.0), (0.0, 0.0), (-1.0, -1.0)]   # top-down only, bottom-up only, the engine's default


def load_matrix(spec):
    kind = spec[len("synth:"):] if spec.startswith("synth:") else None
    if kind == "scircuit":
        rp, ci, va = H.scircuit_like()
    elif kind and kind.startswith("rmat-"):
        rp, ci, va = H.rmat(int(kind.split("-")[1]))
    elif kind and kind.startswith("grid-"):
        rp, ci, va = grid_graph(int(kind.split("-")[1]))
    elif kind and kind.startswith("powerlaw-"):
        _, rows, entries = kind.split("-")
        rp, ci, va = H.powerlaw(int(rows), int(entries))
    elif kind:
        raise SystemExit(f"unknown generator {spec}: synth:grid-<side> | synth:scircuit | synth:rmat-<scale> | synth:powerlaw-<rows>-<entries>")
    else:
        rows, cols, _, rp, ci, va = H.mm_load(spec)
        if rows != cols:
            raise SystemExit("a BFS needs a square matrix")
    return len(rp) - 1, rp, ci, va


def summary(v, scale):
    v = sorted(x / scale for x in v)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def pair_name(p):
    return {FIXED[0]: "top-down", FIXED[1]: "bottom-up", FIXED[2]: "default"}.get(p, f"up={p[0]:g},down={p[1]:g}")


def dump(res):
    """The result as JSON text: one line per top-level field and ONE line per arm (a file stays a few dozen lines)."""
    lines = ["{"] + [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in res.items() if k != "sources"] + [' "sources": {']
    for i, (src, out) in enumerate(res["sources"].items()):
        rest = ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items() if k != "arms")
        lines.append(f"  {json.dumps(src)}: {{{rest}, \"arms\": {{")
        arms = list(out["arms"].items())
        lines += [f"   {json.dumps(k)}: {json.dumps(v)}" + ("," if j + 1 < len(arms) else "") for j, (k, v) in enumerate(arms)]
        lines.append("  }}" + ("," if i + 1 < len(res["sources"]) else ""))
    return "\n".join(lines + [" }", "}"]) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--pairs", default="0.0714:0.0417,0.02:0.0417,0.005:0.0417,0.002:0.0417,0.02:0.01,0.005:0.01,0.002:0.01",
                    help="up_share:down_share, comma-separated (the three fixed points are added)")
    ap.add_argument("--sources", type=int, default=2, help="seeded random sources with non-empty out-lists besides vertex 0")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-levels", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    pairs = FIXED + [tuple(float(x) for x in p.split(":")) for p in args.pairs.split(",") if p]
    n, rp, ci, va = load_matrix(args.matrix)
    vals = (va != 0).astype(np.int32)
    cap = args.max_levels
    inb = (ci >= 0) & (ci < n) & (vals != 0)
    outdeg = np.bincount(ci[inb], minlength=n)
    rng = np.random.default_rng(23)
    cand = np.flatnonzero(outdeg > 0)
    sources = [0] + [int(v) for v in rng.choice(cand, min(args.sources, len(cand)), replace=False)]
    res = {"tool": "tools/bfs_levels_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "max_levels": cap,
           "timing": "device_us: total_ns of the C ABI (events around every step, the set-up launch and the parent pass); "
                     "wall_us_median: the call as the host sees it; median / min / max over the rounds, arms alternating inside a round",
           "sources": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        A = eng.upload_csr(n, n, rp, ci, vals)   # what sh_csr_upload chooses (the environment included)
        eng.synchronize()
        t_up = time.perf_counter() - t0
        F = eng.frontier(A, rp, ci, vals)
        t0 = time.perf_counter()
        G = eng.bfs_graph(rp, ci, vals)
        eng.synchronize()
        t_g = time.perf_counter() - t0
        res.update({"plan": A.describe(), "upload_s": round(t_up, 4), "matrix_footprint_bytes": A.footprint(),
                    "bfs_graph_create_s": round(t_g, 4), "bfs_graph_footprint_bytes": G.footprint, "edges": G.edges})
        xv, yv, sc, lv, pv = eng.alloc(n), eng.alloc(n), eng.alloc(n), eng.alloc(n), eng.alloc(n)
        for source in sources:
            x0 = np.zeros(n, np.int32)
            x0[source] = 1

            def run(arm):
                xv.upload(x0)
                yv.upload(x0)
                eng.synchronize()
                t = time.perf_counter()
                if arm == "sh_iterate":
                    it, cv, per, total = eng.iterate(OR_AND_I32, A, xv, yv, sc, 1, 1, max_iters=cap)
                    r = (it, total)
                elif arm == "sh_iterate_frontier":
                    r = eng.iterate_frontier(OR_AND_I32, A, F, xv, yv, sc, 1, 1, max_iters=cap)
                    r = (r[0], r[6])
                else:
                    pair, with_parent = arm
                    r = eng.bfs_levels(G, xv, lv, pv if with_parent else None, max_levels=cap, up_share=pair[0], down_share=pair[1])
                return r, (time.perf_counter() - t) * 1e6

            # (the parent pass costs the same under every pair: it is timed with the three fixed points only)
            arms = ["sh_iterate", "sh_iterate_frontier"] + [(p, w) for p in pairs for w in (False, True) if not w or p in FIXED]
            (b_it, _), _ = run("sh_iterate")
            reach = xv.download(np.int32) != 0
            want = None
            for arm in arms[1:]:   # warm-up and check
                r, _ = run(arm)
                if arm == "sh_iterate_frontier":
                    continue
                level = lv.download(np.int32)
                if want is None:
                    want = level
                if not np.array_equal(level, want) or not np.array_equal(level >= 0, reach) or r[0] + 1 != b_it or not r[2]:
                    raise SystemExit(f"source {source}, {arm}: levels differ from the first pair's or from sh_iterate's reachability")
            dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
            for _ in range(args.rounds):
                for arm in arms:
                    r, w = run(arm)
                    dev[arm].append(r[1] if isinstance(arm, str) else r[7])
                    wall[arm].append(w)
                    last[arm] = r
            out = {"out_list_length": int(outdeg[source]), "launches_of_sh_iterate": b_it, "arms": {}}
            for arm in arms:
                rec = {"device_us": summary(dev[arm], 1e3), "wall_us_median": round(statistics.median(wall[arm]), 1)}
                if not isinstance(arm, str):
                    pair, with_parent = arm
                    depth, reached, complete, modes, sizes, edges, per, total = last[arm]
                    bu = modes == 1
                    rec.update({"depth": depth, "reached": reached,
                                "steps_top_down": int((~bu).sum()), "steps_bottom_up": int(bu.sum()),
                                "us_per_top_down_step": round(float(per[~bu].sum()) / 1e3 / max(int((~bu).sum()), 1), 3),
                                "us_per_bottom_up_step": round(float(per[bu].sum()) / 1e3 / max(int(bu.sum()), 1), 3),
                                "edges_looked_at": int(edges.sum()),
                                "bottom_up_edges_share_of_graph": round(float(edges[bu].sum()) / max(G.edges * max(int(bu.sum()), 1), 1), 5),
                                "us_outside_the_steps": round((total - float(per.sum())) / 1e3, 3)})
                    if not with_parent and pair == FIXED[2] and len(modes) <= 64:
                        rec["per_level"] = {"mode": [int(m) for m in modes], "size": [int(s) for s in sizes],
                                            "edges": [int(k) for k in edges], "us": [round(float(t) / 1e3, 2) for t in per]}
                name = arm if isinstance(arm, str) else pair_name(arm[0]) + (" +parent" if arm[1] else "")
                out["arms"][name] = rec
            base = out["arms"]["sh_iterate"]["device_us"]["median"]
            fr = out["arms"]["sh_iterate_frontier"]["device_us"]["median"]
            for rec in out["arms"].values():
                rec["device_ratio_vs_sh_iterate"] = round(rec["device_us"]["median"] / base, 4)
                rec["device_ratio_vs_sh_iterate_frontier"] = round(rec["device_us"]["median"] / fr, 4)
            # the pairs of the sweep are kept short: [device_us median, min, max, ratio to sh_iterate, steps top-down, steps bottom-up]
            out["sweep"] = {}
            for p in pairs:
                if p not in FIXED:
                    rec = out["arms"].pop(pair_name(p))
                    out["sweep"][pair_name(p)] = [rec["device_us"]["median"], rec["device_us"]["min"], rec["device_us"]["max"],
                                                  rec["device_ratio_vs_sh_iterate"], rec["steps_top_down"], rec["steps_bottom_up"]]
            res["sources"][str(source)] = out
            print(f"source {source}: " + json.dumps({**{k: (v["device_us"]["median"], v["device_ratio_vs_sh_iterate"])
                                                        for k, v in out["arms"].items()},
                                                     **{k: (v[0], v[3]) for k, v in out["sweep"].items()}}), file=sys.stderr, flush=True)
        # the sweep's verdict: per pair the worst ratio to sh_iterate over the sources (without the parent pass)
        worst = {}
        for p in pairs:
            worst[pair_name(p)] = max(s["arms"][pair_name(p)]["device_ratio_vs_sh_iterate"] if p in FIXED else s["sweep"][pair_name(p)][3]
                                      for s in res["sources"].values())
        res["worst_ratio_vs_sh_iterate_per_pair"] = worst
        for h in (xv, yv, sc, lv, pv, G, F, A):
            h.free()
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(dump(res))


if __name__ == "__main__":
    main()
