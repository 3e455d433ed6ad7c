#!/usr/bin/env python3
"""What sh_scc costs, for one matrix, in one process and with the arms alternating:

  sh_scc                under the four (trim, pivot) settings: total device time, and device time per round kind;
  scc_labels            wall time of the host's single-threaded Tarjan (hostlib.scc_labels) -- the baseline of the total;
  two sh_bfs_levels     from the vertex the pivot round starts from, on the matrix and on its transpose, device times
                        added: the in-project yardstick of a forward and a backward reach, i.e. of the pivot round.  The
                        pivot is the vertex with the largest product of its stored list lengths (ties to the largest
                        index) among the live ones; trimming settles only components of one vertex, so with and without
                        trim it is the same vertex whenever that vertex lies in a component of two or more -- the JSON
                        records the size, and a ratio is given for the trim = 1 arm only then;
  step floor            sh_scc(trim = 0, pivot = 0) on the directed path of 200 vertices (200 colouring rounds, about
                        20 000 steps with next to nothing to do): device time per step.

Method: first every setting's comp is compared with scc_labels' (a difference ends the run); then `--rounds` (>= 5) rounds
over all arms; per arm the median, min and max.

  python tools/scc_bench.py --matrix synth:grid-2048 --out profiles/scc_grid2048.json
  python tools/scc_bench.py --matrix synth:scircuit --out profiles/scc_scircuit.json
  python tools/scc_bench.py --matrix synth:rmat-23 --out profiles/scc_rmat23.json
  python tools/scc_bench.py --matrix synth:powerlaw-10000000-200000000 --out profiles/scc_powerlaw.json

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

SETTINGS = ((1, 1), (1, 0), (0, 1), (0, 0))
KINDS = ("trim", "pivot", "colouring")


def transpose(n, rp, ci, va):
    """The CSR arrays of the transposed matrix (entries with a column outside the matrix dropped: they are no edges)."""
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    keep = (ci >= 0) & (ci < n)
    rows, cols, vals = rows[keep], ci[keep], np.ascontiguousarray(va)[keep]
    order = np.argsort(cols, kind="stable")
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    return t_rp, rows[order], vals[order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va)
    t0 = time.perf_counter()
    want = H.scc_labels(rp, ci, va)
    t_gold = time.perf_counter() - t0
    # the vertex the pivot round starts from when nothing was trimmed: the largest product of the list lengths, ties to the largest index
    edge = (ci >= 0) & (ci < n) & (va.view(np.uint32) != 0)
    rows_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    prod = np.bincount(rows_of[edge], minlength=n).astype(np.uint64) * np.bincount(ci[edge], minlength=n).astype(np.uint64)
    p = int(np.flatnonzero(prod == prod.max()).max())
    p_size = int(np.count_nonzero(want == want[p]))   # >= 2: no trim round can settle p, so every arm's pivot is p
    res = {"tool": "tools/scc_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "components": int(np.count_nonzero(want == np.arange(n))), "largest_component": int(np.bincount(want).max()),
           "pivot_vertex": p, "pivot_component_size": p_size,
           "timing": "device_us: total_ns / ns_per_round of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        t0 = time.perf_counter()
        G = eng.scc_graph(rp, ci, va)
        eng.synchronize()
        res.update({"scc_graph_create_s": round(time.perf_counter() - t0, 4), "scc_graph_footprint_bytes": G.footprint, "edges": G.edges})
        B, Bt = eng.bfs_graph(rp, ci, va), eng.bfs_graph(*transpose(n, rp, ci, va))
        cv, xv, lv = eng.alloc(n), eng.alloc(n), eng.alloc(n)
        pn = 200   # the path pn - 1 -> ... -> 0: entry (r, r + 1)
        Pg = eng.scc_graph(np.minimum(np.arange(pn + 1), pn - 1).astype(np.int32), np.arange(1, pn, dtype=np.int32),
                           np.ones(pn - 1, np.float32))
        pc = eng.alloc(pn)
        x0 = np.zeros(n, np.int32)
        x0[p] = 1
        xv.upload(x0)

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == "scc_labels":
                H.scc_labels(rp, ci, va)
                r = None
            elif arm == "step floor":
                r = eng.scc(Pg, pc, trim=0, pivot=0, max_steps=args.max_steps)
            elif arm == "two sh_bfs_levels":
                r = eng.bfs_levels(B, xv, lv)[7] + eng.bfs_levels(Bt, xv, lv)[7]
            else:
                r = eng.scc(G, cv, trim=arm[0], pivot=arm[1], max_steps=args.max_steps)
            return r, (time.perf_counter() - t) * 1e6

        for arm in SETTINGS:   # warm-up and check, before anything is timed
            r, _ = run(arm)
            if not r[5] or not np.array_equal(cv.download(np.int32), want):
                raise SystemExit(f"trim={arm[0]} pivot={arm[1]}: comp differs from scc_labels'")
        run("two sh_bfs_levels")
        r, _ = run("step floor")
        if not r[5] or r[3] != pn or not np.array_equal(pc.download(np.int32), np.arange(pn)):
            raise SystemExit("step floor: the path did not come out as 200 components in 200 rounds")
        arms = list(SETTINGS) + ["scc_labels", "two sh_bfs_levels", "step floor"]
        floor = []
        dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        per_kind = {a: {k: [] for k in KINDS} for a in SETTINGS}
        for _ in range(args.rounds):
            for arm in arms:
                r, w = run(arm)
                wall[arm].append(w)
                if arm == "step floor":
                    floor.append(r[11] / r[4])
                    last[arm] = r
                elif arm == "two sh_bfs_levels":
                    dev[arm].append(r)
                elif arm != "scc_labels":
                    dev[arm].append(r[11])
                    last[arm] = r
                    for i, k in enumerate(KINDS):
                        per_kind[arm][k].append(int(r[10][r[6] == i].sum()))
        gold = summary(wall["scc_labels"], 1.0)
        yard = summary(dev["two sh_bfs_levels"], 1e3)
        res["arms"]["scc_labels"] = {"wall_us": gold, "first_call_s": round(t_gold, 4)}
        res["arms"]["two sh_bfs_levels"] = {"device_us": yard, "wall_us": summary(wall["two sh_bfs_levels"], 1.0)}
        res["arms"]["step floor"] = {"device_us_per_step": summary(floor, 1e3), "steps": last["step floor"][4], "path_vertices": pn}
        for arm in SETTINGS:
            r = last[arm]
            rec = {"device_us": summary(dev[arm], 1e3), "wall_us": summary(wall[arm], 1.0), "rounds": r[3], "steps": r[4],
                   "trimmed": r[2], "kinds": r[6][:16].tolist(), "sizes": r[7][:16].tolist(), "steps_per_round": r[8][:16].tolist(),
                   "device_us_per_kind": {k: summary(per_kind[arm][k], 1e3) for k in KINDS},
                   "us_per_step": round(float(np.median(dev[arm])) / 1e3 / max(r[4], 1), 3)}
            rec["device_ratio_vs_scc_labels_wall"] = round(rec["device_us"]["median"] / gold["median"], 4)
            rec["wall_ratio_vs_scc_labels_wall"] = round(rec["wall_us"]["median"] / gold["median"], 4)
            if arm[1] and (not arm[0] or p_size >= 2):
                rec["pivot_round_ratio_vs_two_bfs"] = round(rec["device_us_per_kind"]["pivot"]["median"] / max(yard["median"], 1e-9), 4)
            res["arms"][f"sh_scc trim={arm[0]} pivot={arm[1]}"] = rec
        for h in (cv, xv, lv, pc, B, Bt, G, Pg):
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
