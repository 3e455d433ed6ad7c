#!/usr/bin/env python3
"""What sh_rcm costs and what its order does to sh_spmv, for one matrix, in one process and with the arms alternating:

  sh_rcm s<sweeps>      total device time of the call (start, all steps, the closing launch) with sweeps 0 / 2 / 8, the
                        steps, components and root searches, bandwidth and profile before and after, the widest level,
                        the handle's build time and footprint;
  rcm_order s<sweeps>   wall time of the host's single-threaded definition with the same sweeps (hostlib.rcm_order) -- the
                        baseline;
  scipy                 where scipy imports: the bandwidth of scipy.sparse.csgraph.reverse_cuthill_mckee on the
                        symmetrised pattern, beside ours (its ties and its root differ, so only the bandwidths compare);
  spmv                  the point of the tool: the matrix as given and as permuted by perm (rows and columns, on the host:
                        B = A[perm][:, perm]) are uploaded under the default plan, and sh_spmv (plus-times, float32) is
                        timed on both in this process, in blocks that alternate between the two.

--shuffle relabels the vertices by a seeded permutation first (what a matrix looks like when its numbering carries no
locality).  The graph is the simple undirected graph under the matrix' entries, so a directed generator's output needs no
symmetrising first.

Method: first perm, pos, level, the components, the searches, bandwidth and profile and the record of every step of every
arm are compared with the host gold's (==; a difference ends the run), and both SpMV results with a float64 product on
the host; then `--rounds` (>= 5) rounds over all arms; per arm the median, min and max.  One process; run it under
`timeout`:

  timeout -k 10 900 python tools/rcm_bench.py --matrix synth:grid-2048 --out profiles/rcm_grid2048.json
  timeout -k 10 900 python tools/rcm_bench.py --matrix synth:grid-2048 --shuffle --out profiles/rcm_grid2048_shuffled.json
  timeout -k 10 900 python tools/rcm_bench.py --matrix synth:rmat-18 --out profiles/rcm_rmat18.json
  timeout -k 10 900 python tools/rcm_bench.py --matrix synth:scircuit --out profiles/rcm_scircuit.json

One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparseharness_amd import abi  # noqa: E402
from sparseharness_amd import hostlib as H  # noqa: E402
from sparseharness_amd.engine import Engine  # noqa: E402

from bfs_levels_bench import load_matrix, summary  # noqa: E402  (tools/ is the script's directory)

SEED = 0x5EED
SWEEPS = (0, 2, 8)
STEP_CAP = 1 << 20   # the per-step arrays of a call have this many places at most (the binding's own cap)


def relabelled(n, rp, ci, va, name):
    """The matrix with row r as row name[r] and column c as column name[c]; every row's entries in ascending column."""
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    r2, c2 = name[row], name[ci]
    order = np.lexsort((c2, r2))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int32)
    return rp2, c2[order].astype(np.int32), np.ascontiguousarray(va[order])


def product(n, rp, ci, va, x):
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    return np.bincount(row, weights=va.astype(np.float64) * x[ci].astype(np.float64), minlength=n)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", default="synth:grid-2048")
    ap.add_argument("--shuffle", action="store_true", help="relabel the vertices by a seeded permutation first")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spmv-block", type=int, default=50, help="sh_spmv calls per block of the SpMV leg")
    ap.add_argument("--spmv-blocks", type=int, default=7, help="blocks per matrix, alternating")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("--rounds: at least 5")
    n, rp, ci, va = load_matrix(args.matrix)
    rp, ci, va = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float32)
    if ((ci < 0) | (ci >= n)).any():
        raise SystemExit("a column outside the matrix: the SpMV leg permutes rows and columns alike")
    if args.shuffle:
        rp, ci, va = relabelled(n, rp, ci, va, np.random.default_rng(SEED).permutation(n))
    res = {"tool": "tools/rcm_bench.py", "matrix": args.matrix, "shuffled": bool(args.shuffle), "rows": n, "entries": int(rp[-1]),
           "rounds": args.rounds, "seed": SEED,
           "timing": "device_us: total_ns of the C ABI (hipEvent); wall_us: the call as the host sees it; gold_wall_us: "
                     "hostlib.rcm_order; median / min / max over the rounds, arms alternating inside a round; spmv: device ns "
                     "of sh_spmv (hipEvent), the median of every block of calls, blocks alternating between the two matrices",
           "arms": {}}
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        A = sp.csr_matrix((np.ones(len(ci), np.float32), ci, rp), shape=(n, n))
        A = (A + A.T).tocsr()
        p = np.asarray(reverse_cuthill_mckee(A, symmetric_mode=True), np.int64)
        inv = np.empty(n, np.int64)
        inv[p] = np.arange(n)
        coo = A.tocoo()
        res["scipy_bandwidth_after"] = int(np.abs(inv[coo.row] - inv[coo.col]).max()) if coo.nnz else 0
    except ImportError:
        pass
    with Engine(args.device) as eng:
        res["device"] = eng.device_name
        eng.synchronize()
        t0 = time.perf_counter()
        G = eng.rcm_graph(rp, ci, va)
        eng.synchronize()
        res.update({"rcm_graph_create_s": round(time.perf_counter() - t0, 4), "rcm_graph_footprint_bytes": G.footprint,
                    "edges": G.edges, "max_degree": G.max_degree})
        pv, qv, lv = (eng.alloc(max(n, 1)) for _ in range(3))

        def device(sweeps):
            eng.synchronize()
            t = time.perf_counter()
            r = eng.rcm_order(G, pv, qv, lv, sweeps=sweeps, max_steps=min((sweeps + 2) * n + 1, STEP_CAP))
            return r, (time.perf_counter() - t) * 1e6

        # warm-up and check, before anything is timed
        dev, wall, gold_wall, last, perms = ({s: [] for s in SWEEPS} for _ in range(5))
        for s in SWEEPS:
            for v in (pv, qv, lv):
                v.fill(7, np.int32)
            g = H.rcm_order(rp, ci, va, sweeps=s, records=True)
            r, _ = device(s)
            if not r[3]:
                raise SystemExit(f"s{s}: the run was cut short at {r[2]} steps")
            if (r[0], r[1]) != (g[7], g[8]) or r[4:8] != g[3:7]:
                raise SystemExit(f"s{s}: components, searches, bandwidth or profile differ from rcm_order's")
            for name, v, ref in (("perm", pv, g[0]), ("pos", qv, g[1]), ("level", lv, g[2])):
                if n and not np.array_equal(v.download(np.int32, n), ref):
                    raise SystemExit(f"s{s}: {name} differs from rcm_order's")
            for name, a, b in (("kind", r[8], g[9]), ("size", r[9], g[10]), ("edges", r[10], g[11])):
                if not np.array_equal(a, b):
                    raise SystemExit(f"s{s}: {name}_per_step differs from rcm_order's")
            last[s], perms[s] = r, g[0]
        for _ in range(args.rounds):
            for s in SWEEPS:
                r, w = device(s)
                dev[s].append(r[-1])
                wall[s].append(w)
                last[s] = r
                t = time.perf_counter()
                H.rcm_order(rp, ci, va, sweeps=s)
                gold_wall[s].append((time.perf_counter() - t) * 1e6)
        for s in SWEEPS:
            r = last[s]
            gold = summary(gold_wall[s], 1.0)
            rec = {"device_us": summary(dev[s], 1e3), "wall_us": summary(wall[s], 1.0), "gold_wall_us": gold, "samples": len(dev[s]),
                   "components": r[0], "searches": r[1], "steps": r[2], "bandwidth_before": r[4], "bandwidth_after": r[5],
                   "profile_before": r[6], "profile_after": r[7], "numbering_steps": int((r[8] == 1).sum()),
                   "widest_level": int(r[9].max()) if r[2] else 0, "list_entries_walked": int(r[10].sum()),
                   "step_us_median": round(float(np.median(r[11])) / 1e3, 1) if r[2] else 0.0}
            rec["device_ratio_vs_gold_wall"] = round(rec["device_us"]["median"] / gold["median"], 5)
            res["arms"]["s%d" % s] = rec
        for h in (pv, qv, lv, G):
            h.free()

        # the SpMV leg: the matrix as given against the matrix in the new order (sweeps = 8)
        perm = perms[SWEEPS[-1]].astype(np.int64)
        pos = np.empty(n, np.int64)
        pos[perm] = np.arange(n)
        rp2, ci2, va2 = relabelled(n, rp, ci, va, pos)
        x = np.random.default_rng(SEED + 1).random(n, dtype=np.float32)
        mats = {"original": (rp, ci, va, x), "reordered": (rp2, ci2, va2, np.ascontiguousarray(x[perm]))}
        held, times = {}, {k: [] for k in mats}
        for k, (a, b, c, xv) in mats.items():
            A = eng.upload_csr(n, n, a, b, c)
            xd, yd = eng.vector(xv), eng.alloc(max(n, 1))
            for _ in range(10):
                eng.spmv(abi.PLUS_TIMES_F32, A, xd, None, 1.0, 0.0, yd)
            y, want = yd.download(np.float32, n), product(n, a, b, c, xv)
            if not np.allclose(y, want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max() if n else 0)):
                raise SystemExit(f"spmv on the {k} matrix differs from the float64 product")
            held[k] = (A, xd, yd)
        for _ in range(args.spmv_blocks):
            for k, (A, xd, yd) in held.items():
                ns = [eng.spmv(abi.PLUS_TIMES_F32, A, xd, None, 1.0, 0.0, yd, timed=True) for _ in range(args.spmv_block)]
                times[k].append(float(np.median(ns)))
        res["spmv"] = {k: summary(v, 1e3) for k, v in times.items()}
        res["spmv"].update({"unit": "us per sh_spmv", "calls_per_block": args.spmv_block, "blocks": args.spmv_blocks,
                            "reordered_over_original": round(res["spmv"]["reordered"]["median"] / res["spmv"]["original"]["median"], 4)})
        for A, xd, yd in held.values():
            for h in (xd, yd, A):
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
