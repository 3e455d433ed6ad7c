#!/usr/bin/env python3
"""What sh_wcc costs, for one matrix, in one process and with the arms alternating:

  sh_wcc sample=s       s in {0, 1, 2, 4} on the matrix as it is (directed where it is): total device time, the rounds,
                        the vertices skipped, the entries looked at;
  wcc_labels            wall time of the host's single-threaded union-find (hostlib.wcc_labels) -- the baseline;
  sh_scc                with trim and pivot on, on the SYMMETRIC pattern (the matrix itself where it is symmetric, else
                        the matrix plus its transpose), where strong and weak components are the same: the only call
                        that answered the question before sh_wcc;
  sh_wcc (symmetric)    sample = 2 on that same symmetric pattern, when it is not the matrix itself: the like-for-like
                        partner of the sh_scc arm.

Method: first every arm's comp is compared with wcc_labels' (a difference ends the run); then `--rounds` (>= 5) rounds
over all arms; per arm the median, min and max.

  python tools/wcc_bench.py --matrix synth:grid-2048 --out profiles/wcc_grid2048.json
  python tools/wcc_bench.py --matrix synth:scircuit --out profiles/wcc_scircuit.json
  python tools/wcc_bench.py --matrix synth:rmat-23 --out profiles/wcc_rmat23.json

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

SAMPLES = (0, 1, 2, 4)


def symmetric_pattern(n, rp, ci, va):
    """-> (is_symmetric, rp, ci, va): the edges of the matrix plus their transposes, values 1 (row r: its in-list, then
    its out-list; parallel edges stay).  When the edge set is symmetric already, the matrix itself."""
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    keep = (ci >= 0) & (ci < n) & (np.ascontiguousarray(va).view(np.uint32) != 0)
    rows, cols = rows[keep], ci[keep]
    n_in, n_out = np.bincount(rows, minlength=n), np.bincount(cols, minlength=n)
    if np.array_equal(n_in, n_out):   # (cheap, and enough to tell a directed generator's output; then the edge sets themselves)
        a, b = rows.astype(np.int64) * n + cols, cols.astype(np.int64) * n + rows
        if np.array_equal(np.unique(a), np.unique(b)):
            return True, rp, ci, va
        del a, b
    order = np.argsort(cols, kind="stable")
    s_rp = np.concatenate([[0], np.cumsum(n_in + n_out)]).astype(np.int64)
    in_rp = np.concatenate([[0], np.cumsum(n_in)]).astype(np.int64)
    out_rp = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
    s_ci = np.empty(2 * len(rows), np.int32)
    s_ci[np.arange(len(rows)) + np.repeat(s_rp[:-1] - in_rp[:-1], n_in)] = cols
    s_ci[np.arange(len(rows)) + np.repeat(s_rp[:-1] + n_in - out_rp[:-1], n_out)] = rows[order]
    return False, s_rp.astype(np.int32), s_ci, np.ones(len(s_ci), np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=1 << 16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    va = np.ascontiguousarray(va)
    t0 = time.perf_counter()
    want = H.wcc_labels(rp, ci, va)
    t_gold = time.perf_counter() - t0
    is_sym, s_rp, s_ci, s_va = symmetric_pattern(n, rp, ci, va)
    if n * 2 + len(s_ci) >= (1 << 31) - 256:
        raise SystemExit("the symmetric pattern has too many entries for a handle")
    sizes = np.bincount(want)
    res = {"tool": "tools/wcc_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "rounds": args.rounds,
           "components": int(np.count_nonzero(want == np.arange(n))), "largest_component": int(sizes.max()),
           "matrix_is_symmetric": bool(is_sym), "symmetric_pattern_entries": int(len(s_ci)),
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round", "arms": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        t0 = time.perf_counter()
        G = eng.wcc_graph(rp, ci, va)
        eng.synchronize()
        res.update({"wcc_graph_create_s": round(time.perf_counter() - t0, 4), "wcc_graph_footprint_bytes": G.footprint, "edges": G.edges})
        Gs = G if is_sym else eng.wcc_graph(s_rp, s_ci, s_va)
        Sg = eng.scc_graph(s_rp, s_ci, s_va)
        res["scc_graph_footprint_bytes"] = Sg.footprint
        cv = eng.alloc(n)
        arms = [f"sh_wcc sample={s}" for s in SAMPLES] + ["wcc_labels", "sh_scc (symmetric)"] + ([] if is_sym else ["sh_wcc sample=2 (symmetric)"])

        def run(arm):
            eng.synchronize()
            t = time.perf_counter()
            if arm == "wcc_labels":
                H.wcc_labels(rp, ci, va)
                r = None
            elif arm == "sh_scc (symmetric)":
                r = eng.scc(Sg, cv)
            elif arm == "sh_wcc sample=2 (symmetric)":
                r = eng.wcc(Gs, cv, sample=2, max_rounds=args.max_rounds)
            else:
                r = eng.wcc(G, cv, sample=int(arm.split("=")[1]), max_rounds=args.max_rounds)
            return r, (time.perf_counter() - t) * 1e6

        for arm in arms:   # warm-up and check, before anything is timed
            if arm == "wcc_labels":
                continue
            r, _ = run(arm)
            done = r[5] if arm.startswith("sh_scc") else r[3]
            if not done or not np.array_equal(cv.download(np.int32), want):
                raise SystemExit(f"{arm}: comp differs from wcc_labels'")
        dev, wall, last = {a: [] for a in arms}, {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for arm in arms:
                r, w = run(arm)
                wall[arm].append(w)
                if r is not None:
                    dev[arm].append(r[11] if arm.startswith("sh_scc") else r[9])
                    last[arm] = r
        gold = summary(wall["wcc_labels"], 1.0)
        res["arms"]["wcc_labels"] = {"wall_us": gold, "first_call_s": round(t_gold, 4)}
        for arm in arms:
            if arm == "wcc_labels":
                continue
            r = last[arm]
            rec = {"device_us": summary(dev[arm], 1e3), "wall_us": summary(wall[arm], 1.0)}
            if arm.startswith("sh_scc"):
                rec.update({"rounds": r[3], "steps": r[4], "kinds": r[6][:8].tolist(), "sizes": r[7][:8].tolist()})
            else:
                rec.update({"rounds": r[2], "skipped": r[1], "kinds": r[4][:16].tolist(), "hooks": r[5][:16].tolist(),
                            "jumps": r[6][:16].tolist(), "edges_looked_at": r[7][:16].tolist(),
                            "us_per_round": [round(x / 1e3, 1) for x in r[8][:16].tolist()]})
            rec["device_ratio_vs_wcc_labels_wall"] = round(rec["device_us"]["median"] / gold["median"], 4)
            rec["wall_ratio_vs_wcc_labels_wall"] = round(rec["wall_us"]["median"] / gold["median"], 4)
            res["arms"][arm] = rec
        scc_med = res["arms"]["sh_scc (symmetric)"]["device_us"]["median"]
        partner = "sh_wcc sample=2" if is_sym else "sh_wcc sample=2 (symmetric)"
        res["sh_wcc_sample2_vs_sh_scc_same_pattern"] = round(res["arms"][partner]["device_us"]["median"] / max(scc_med, 1e-9), 4)
        for h in [cv, Sg, G] + ([] if is_sym else [Gs]):
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
