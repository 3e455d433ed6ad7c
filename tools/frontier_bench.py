#!/usr/bin/env python3
"""What recomputing only the rows whose inputs changed buys: for one matrix, SSSP (SH_MIN_PLUS_F32, alpha = beta = 0) and
BFS (SH_OR_AND_I32, alpha = beta = 1) from vertex 0 to convergence, in the same process and alternating:

  baseline   sh_iterate under the plan sh_csr_upload chooses by default;
  frontier   sh_iterate_frontier on the same upload at dense_share = 0 (every launch dense: sh_iterate plus the change
             detection), a sweep of shares, 1 (every launch from 2 on sparse), and the engine's default (-1).

Method: one warm-up of every arm (its result and launch count are compared with the baseline's), then `--rounds`
(>= 5) rounds over all arms; per arm the median, min and max of the total device time (events around each launch, the
total_ns of the C ABI) and of the wall time of the call.  The baseline's own min / max is the margin any comparison
has to clear.  Also recorded: launches by mode, rows recomputed, device time per dense / per sparse launch, the time
sh_frontier_create takes (transpose build on the device) and the handle's footprint next to sh_csr_upload's.

  python tools/frontier_bench.py --matrix synth:grid-2048 --out profiles/frontier_grid2048.json
  python tools/frontier_bench.py --matrix synth:scircuit --out profiles/frontier_scircuit.json
  python tools/frontier_bench.py --matrix synth:rmat-23 --out profiles/frontier_rmat23.json

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
from sparseharness_amd.engine import MIN_PLUS_F32, OR_AND_I32, Engine  # noqa: E402


def grid_graph(side, seed=5):
    """4-neighbour grid of side x side vertices, vertex (i, j) = i * side + j, integer weights 1..16."""
    idx = np.arange(side * side, dtype=np.int64).reshape(side, side)
    src, dst = [], []
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        src += [a.ravel(), b.ravel()]
        dst += [b.ravel(), a.ravel()]
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.argsort(src * (side * side) + dst, kind="stable")
    src, dst = src[order], dst[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=side * side))]).astype(np.int32)
    va = np.random.default_rng(seed).integers(1, 17, len(dst)).astype(np.float32)
    return rp, dst.astype(np.int32), va


def load_matrix(spec):
    kind = spec[len("synth:"):] if spec.startswith("synth:") else None
    if kind == "scircuit":
        rp, ci, va = H.scircuit_like()
    elif kind and kind.startswith("rmat-"):
        rp, ci, va = H.rmat(int(kind.split("-")[1]))
    elif kind and kind.startswith("grid-"):
        rp, ci, va = grid_graph(int(kind.split("-")[1]))
    elif kind:
        raise SystemExit(f"unknown generator {spec}: synth:grid-<side> | synth:scircuit | synth:rmat-<scale>")
    else:
        rows, cols, _, rp, ci, va = H.mm_load(spec)
        if rows != cols:
            raise SystemExit("the iteration needs a square matrix")
    return len(rp) - 1, rp, ci, va


def summary(v, scale):
    v = sorted(x / scale for x in v)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:scircuit")
    ap.add_argument("--shares", default="0,0.001,0.005,0.02,0.1,0.3,1,-1")
    ap.add_argument("--apps", default="sssp,bfs")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=20000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    shares = [float(s) for s in args.shares.split(",")]
    n, rp, ci, va = load_matrix(args.matrix)
    cap = args.max_iters
    res = {"tool": "tools/frontier_bench.py", "matrix": args.matrix, "rows": n, "entries": int(rp[-1]), "source": 0,
           "rounds": args.rounds, "max_iters": cap,
           "timing": "device_us: events around each launch (total_ns of the C ABI); wall_us: the call as the host sees it; "
                     "median / min / max over the rounds, arms alternating inside a round",
           "apps": {}}
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        for app in args.apps.split(","):
            sr, a, b = (MIN_PLUS_F32, 0.0, 0.0) if app == "sssp" else (OR_AND_I32, 1, 1)
            vals = va.astype(np.float32) if app == "sssp" else (va != 0).astype(np.int32)
            dt = vals.dtype
            x0 = np.full(n, np.float32(3.4028235e38), np.float32) if app == "sssp" else np.zeros(n, np.int32)
            x0[0] = 0 if app == "sssp" else 1
            eng.synchronize()
            t0 = time.perf_counter()
            A = eng.upload_csr(n, n, rp, ci, vals)   # what sh_csr_upload chooses (the environment included)
            eng.synchronize()
            t_up = time.perf_counter() - t0
            t0 = time.perf_counter()
            F = eng.frontier(A, rp, ci, vals)
            eng.synchronize()
            t_fr = time.perf_counter() - t0
            xv, yv, sc = eng.alloc(n), eng.alloc(n), eng.alloc(n)

            def run(share):
                xv.upload(x0)
                yv.upload(x0)
                eng.synchronize()
                t = time.perf_counter()
                if share is None:
                    it, cv, per, total = eng.iterate(sr, A, xv, yv, sc, a, b, max_iters=cap)
                    r = (it, cv, [0] * it, None, [n] * it, per, total)
                else:
                    r = eng.iterate_frontier(sr, A, F, xv, yv, sc, a, b, max_iters=cap, dense_share=share)
                return r, (time.perf_counter() - t) * 1e6

            arms = [None] + shares
            (b_it, b_cv, *_), _ = run(None)
            want = xv.download(dt)
            for s in shares:   # warm-up and check
                (it, cv, *_), _ = run(s)
                if (it, cv) != (b_it, b_cv) or not np.array_equal(xv.download(dt).view(np.uint32), want.view(np.uint32)):
                    raise SystemExit(f"{app}: dense_share {s} differs from sh_iterate ({it}, {cv}) vs ({b_it}, {b_cv})")
            dev, wall, last = {s: [] for s in arms}, {s: [] for s in arms}, {}
            for _ in range(args.rounds):
                for s in arms:
                    r, w = run(s)
                    dev[s].append(r[6])
                    wall[s].append(w)
                    last[s] = r
            out = {"launches": b_it, "converged": b_cv, "plan": A.describe(), "upload_s": round(t_up, 4),
                   "matrix_footprint_bytes": A.footprint(), "frontier_create_s": round(t_fr, 4),
                   "frontier_footprint_bytes": F.footprint(), "arms": {}}
            for s in arms:
                it, cv, modes, changed, active, per, total = last[s]
                n_sparse = sum(modes)
                t_sparse = sum(t for t, m in zip(per, modes) if m)
                t_dense = sum(t for t, m in zip(per, modes) if not m)
                out["arms"]["sh_iterate" if s is None else f"dense_share={s:g}"] = {
                    "device_us": summary(dev[s], 1e3), "wall_us": summary(wall[s], 1.0),
                    "dense_launches": it - n_sparse, "sparse_launches": n_sparse,
                    "us_per_dense_launch": round(t_dense / 1e3 / max(it - n_sparse, 1), 3),
                    "us_per_sparse_launch": round(t_sparse / 1e3 / max(n_sparse, 1), 3),
                    "rows_recomputed": int(sum(active)), "rows_recomputed_share": round(sum(active) / (max(it, 1) * n), 5),
                    "max_changed_rows": int(max(changed)) if changed else None,
                }
            base = out["arms"]["sh_iterate"]
            for name, arm in out["arms"].items():
                arm["device_ratio_vs_sh_iterate"] = round(arm["device_us"]["median"] / base["device_us"]["median"], 4)
                arm["wall_ratio_vs_sh_iterate"] = round(arm["wall_us"]["median"] / base["wall_us"]["median"], 4)
            res["apps"][app] = out
            print(f"{app}: {json.dumps(out)}", file=sys.stderr, flush=True)
            for h in (xv, yv, sc, F, A):
                h.free()
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
