#!/usr/bin/env python3
"""bench.py -- headline benchmark of the SpMV hot path (BASELINE.json metric).

A "step" is one float (+,x) CSR SpMV  out = A x  (alpha=1, beta=0, the
configuration of the reference's app/spmv.cpp:117-120) over the whole synthetic
matrix, inputs resident in HBM.  Default workload = BASELINE.json configs[4],
the one the target is quoted on: power-law 10 M rows / 200 M non-zeros
(SURVEY.md 8d generator, seed 0x5EED1000), which fits one GPU.

Multi-GPU (one rank per GPU; `python bench.py --gpus N` starts the ranks itself through
torch.distributed.run when no launcher did): the SAME matrix is row-sharded into
work-balanced contiguous row ranges (strong scaling); x is replicated; single-shot
SpMV needs no collective (each rank owns its slice of y).
value = 2 * nnz_total * K / max-over-ranks wall time.

A plain run sets up, warms up, times the --steps steps, writes the output of the
last timed step if --dump-outputs DIR is given (DIR/y.npy, float32: y of every row;
past 64 MB a fixed seeded sample of rows, with their indices in DIR/y_rows.npy) and
prints ONE JSON line on rank 0 with the driver's contract keys plus
  roofline     : algorithmic bytes of this rank's launch / its average device
                 time (HIP events on the launch stream), vs 8 TB/s HBM peak
--full adds what takes runs or checks of its own (the keys are null without it):
  parity       : the timed output against the oracle's gold
  cpu_baseline : the oracle's restatement of the reference gold dot loop
                 (inc/spmv_gold.h:17-26) timed on this host (N=1 only): single thread
                 (the reference is single-threaded) and, under all_cores, row-parallel
                 on every host core
  frac_raw_values : the same matrix with value coding off (general fp32 data)
  frac_dict16_values : the same matrix with 976 distinct weights (two-byte dictionary codes)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md

# HBM bytes per SpMV launch come from SEPARATE rocprofv3 --pmc passes (FETCH_SIZE x2 correction +
# WRITE_SIZE, MI355X_MICROARCH.md "HBM"; tools/pmc.sh): PMC cannot be collected inside this process.
# profiles/measured_traffic.json holds one record per (workload, device layout, n_gpus); a run whose
# layout string has no record reports null -- the figure never outlives the kernels it was measured on.
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "measured_traffic.json")


def measured_traffic(workload, layout, n_gpus):
    try:
        recs = json.load(open(TRAFFIC_FILE))
    except (OSError, ValueError):
        return None, "no profiles/measured_traffic.json"
    for r in recs:
        if (r["workload"], r["layout"], r["n_gpus"]) == (workload, layout, n_gpus):
            return r["bytes"], r["source"]
    return None, "no rocprofv3 --pmc record for this workload / layout in profiles/measured_traffic.json"

WORKLOADS = {
    # name: (kind, rows, nnz, description)
    "powerlaw-10M-200M": ("powerlaw", 10_000_000, 200_000_000,
                          "power-law rows P(d)~d^-2.1 on [1,1e6], uniform columns, 10M x 10M, 200M nnz, seed 0x5EED1000"),
    "rmat-23": ("rmat", 1 << 23, 16 << 23, "Graph500 R-MAT scale 23, edge factor 16, permuted ids, seed 0x5EED0023"),
    # NOT a BASELINE config: the same R-MAT without the vertex permutation, i.e. a graph whose columns are
    # as local as R-MAT's quadrant recursion makes them -- what the plans reach when there IS column locality
    "rmat-23-unpermuted": ("rmat-local", 1 << 23, 16 << 23,
                           "Graph500 R-MAT scale 23, edge factor 16, ids NOT permuted (column locality), seed 0x5EED0023"),
    "scircuit-like": ("scircuit", 170_998, 958_936, "scircuit-shaped stand-in, seed 0x5EED5C1C"),
}


def make_workload(name, rows=None, nnz=None):
    from sparseharness_amd import hostlib as H
    kind, r, z, desc = WORKLOADS[name]
    if kind == "powerlaw":
        r, z = rows or r, nnz or z
        rp, ci, va = H.powerlaw(r, z)
        if rows or nnz:
            desc += f" [overridden to {r} rows / {z} nnz]"
    elif kind in ("rmat", "rmat-local"):
        scale = int(np.log2(rows)) if rows else 23
        rp, ci, va = H.rmat(scale, permute=(kind == "rmat"))
        r, z = 1 << scale, int(rp[-1])
    else:
        rp, ci, va = H.scircuit_like()
    return rp, ci, va, r, desc


def usable_host_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota
    (a GPU box hands a one-GPU job 16 of its 256 cores; more threads than that only thrash)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota, period = txt[0], float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota not in ("max", "-1"):
                n = max(1, min(n, int(float(quota) / period + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def self_launch(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks as fresh child processes
    (torch.distributed.run, one per GPU) BEFORE this process has imported torch or touched HIP -- a process
    that has initialised the GPU must never exec -- relay their output (rank 0 prints the JSON line) and
    exit with their return code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(path, y, world, rank):
    """--dump-outputs: y of the last timed step, every row (rank 0 gathers the other ranks' slices), as
    DIR/y.npy in float32; past DUMP_LIMIT_BYTES a fixed, seeded sample of rows, their indices in DIR/y_rows.npy."""
    if world > 1:
        import torch.distributed as dist
        parts = [None] * world if rank == 0 else None
        dist.gather_object(y, parts, dst=0)
        if rank != 0:
            return
        y = np.concatenate(parts)
    os.makedirs(path, exist_ok=True)
    y = np.ascontiguousarray(y, np.float32)
    if y.nbytes > DUMP_LIMIT_BYTES:
        k = (DUMP_LIMIT_BYTES - 4096) // (4 + 8)
        rows = np.sort(np.random.default_rng(0x5EED).choice(len(y), k, replace=False))
        np.save(os.path.join(path, "y_rows.npy"), rows.astype(np.float64))
        y = y[rows]
    np.save(os.path.join(path, "y.npy"), y)


def oracle_legs(args, rp, ci, va, s_rp, s_ci, s_va, x_host, y, n, nnz_total, rank, world):
    """--full: this rank's rows of the timed output against the oracle's gold -> (cpu_baseline, parity, mismatches);
    on a single rank the gold is the timed single-thread / all-cores CPU baseline."""
    from oracle import oracle as O   # checker + reported CPU baseline only
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        gold = np.empty(n, np.float32)
        times = []
        for _ in range(3):
            tc = time.perf_counter()
            O.gold_dot(rp, ci, va, x_host, 1.0, out=gold)
            times.append(time.perf_counter() - tc)
        tmed = sorted(times)[1]
        # the same loop row-parallel on every host core this process may use (OpenMP, rows still summed sequentially)
        ncores = usable_host_cores()
        par = np.empty(n, np.float32)
        ptimes, used = [], 1
        for _ in range(3):
            tc = time.perf_counter()
            _, used = O.gold_dot_all_cores(rp, ci, va, x_host, 1.0, out=par, threads=ncores)
            ptimes.append(time.perf_counter() - tc)
        pmed = sorted(ptimes)[1]
        model = ""
        try:
            model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
        except (OSError, StopIteration):
            pass
        cpu = {"value": round(2.0 * nnz_total / tmed / 1e9, 4), "unit": "GFLOP/s", "cores": 1, "kind": "port",
               "sample": f"full {args.workload} matrix ({nnz_total} nnz), median of 3 single-thread runs of the "
                         f"gold dot loop restatement (oracle_gold_dot_f32), {tmed:.3f} s each",
               "all_cores": {"value": round(2.0 * nnz_total / pmed / 1e9, 4), "unit": "GFLOP/s", "cores": used,
                             "sample": f"the same loop, rows dealt to {used} OpenMP threads (oracle_gold_dot_f32_omp), "
                                       f"median of 3, {pmed:.3f} s each",
                             "same_bits_as_single_thread": bool(np.array_equal(par.view(np.uint32), gold.view(np.uint32)))},
               "host_cpus": os.cpu_count(), "cpu_model": model}
        want = gold
    else:
        want = O.gold_dot(s_rp, s_ci, s_va, x_host, 1.0)
    tol = 1e-5 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    off = np.nonzero(np.abs(y.astype(np.float64) - want.astype(np.float64)) > tol)[0]
    # A row whose partial sums pass 2^24 is summed inexactly by the sequential float gold itself
    # (error ~ n*2^-24); there the GPU's tree order legitimately differs by more than 1e-5.  Such a row
    # is accepted only if the GPU value is within 1e-5 of the exact (float64) dot AND no farther from it
    # than the gold is.  Everything else is a mismatch.
    bad, excused = 0, 0
    chk_rp, chk_ci, chk_va = (rp, ci, va) if (rank == 0 and world == 1 and not args.no_cpu_baseline) else (s_rp, s_ci, s_va)
    for r in off:
        a, b = int(chk_rp[r]), int(chk_rp[r + 1])
        terms = x_host[chk_ci[a:b]].astype(np.float64) * chk_va[a:b].astype(np.float64)
        exact = terms.sum()
        # (non-integer weights: every row rounds, in gold and on the GPU alike; the yardstick is then the exact dot)
        if ((np.abs(terms).sum() >= 2 ** 24 or args.real_values) and abs(y[r] - exact) <= 1e-5 * max(1.0, abs(exact))
                and (abs(y[r] - exact) <= abs(want[r] - exact) or args.real_values)):
            excused += 1
        else:
            bad += 1
    parity = {"checked_rows": len(y), "mismatches_rel_1e-5": bad,
              "rows_where_gold_itself_is_inexact_and_gpu_is_closer_to_exact": excused,
              "bit_exact_rows": int((y == want).sum())}
    return cpu, parity, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="powerlaw-10M-200M", choices=sorted(WORKLOADS))
    ap.add_argument("--rows", type=int, default=None, help="override size (testing only; makes the number non-headline)")
    ap.add_argument("--nnz", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="also check the output against the oracle and run the extra legs (CPU baseline, other value codings)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the output of the last timed step to DIR/y.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-ablation", action="store_true",
                    help="with --full: skip the extra timing of the same matrix with other value codings (N=1 only)")
    ap.add_argument("--traffic-bytes", type=float, default=None,
                    help="HBM bytes per launch from a separate rocprofv3 --pmc pass (corrected); echoed into roofline.traffic")
    ap.add_argument("--real-values", action="store_true",
                    help="replace the integer weights by non-integer floats (~1e6 distinct values: no value coding possible)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)

    import torch
    import torch.distributed as dist
    from sparseharness_amd import partition
    from sparseharness_amd.engine import PLUS_TIMES_F32, Engine

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the SpMV engine has no CPU fallback")
    # SH_BENCH_REHEARSAL=1: every rank on GPU 0 over gloo -- exercises the N > 1 code path (sharding, barriers,
    # max-over-ranks) on a one-GPU box; its timings mean nothing and the line says so
    rehearsal = os.environ.get("SH_BENCH_REHEARSAL") == "1"
    dev_index = 0 if rehearsal else local_rank
    torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))

    t_gen = time.time()
    rp, ci, va, n, desc = make_workload(args.workload, args.rows, args.nnz)
    if args.real_values:
        # weights w + (k mod 997) / 1024: exactly representable, > 256 distinct values, sums exact in float64
        va = (va + (np.arange(len(va), dtype=np.int64) % 997).astype(np.float32) / np.float32(1024)).astype(np.float32)
        desc += " [weights made non-integer: w + (k mod 997)/1024]"
    nnz_total = int(rp[-1])
    t_gen = time.time() - t_gen

    # ---- shard: nnz-balanced contiguous row ranges
    bounds = partition.row_bounds(rp, world, cols=n)   # ranges of equal estimated HBM work
    r0, r1 = int(bounds[rank]), int(bounds[rank + 1])
    s_rp, s_ci, s_va = partition.take_rows(rp, ci, va, r0, r1)
    s_rows, s_nnz = r1 - r0, int(s_rp[-1])

    stream = torch.cuda.current_stream()
    eng = Engine(dev_index, stream=stream.cuda_stream)
    # (a first, small upload loads the code objects of the layout builders, so that upload_seconds is the upload itself)
    # (skipped for an older engine build under test -- SH_LIB + SH_LIB_PARTIAL=1, tools/kstats_arms.sh / ab_probe.py: the
    # options struct of this ABI version would be read as that build's older one)
    if not (os.environ.get("SH_LIB") and os.environ.get("SH_LIB_PARTIAL") == "1"):
        w_rp = np.arange(0, 4097 * 8, 8, dtype=np.int32)
        eng.upload_csr(4096, 4096, w_rp, (np.arange(4096 * 8, dtype=np.int32) * 7) % 4096, np.ones(4096 * 8, np.float32), plan=2, build=2).free()
    t_up = time.time()
    A = eng.upload_csr(s_rows, n, s_rp, s_ci, s_va)
    t_up = time.time() - t_up
    x_host = (1 + np.arange(n) % 7).astype(np.float32)  # a wrong gather cannot pass
    x_t = torch.from_numpy(x_host).cuda()
    out_t = torch.zeros(max(s_rows, 1), dtype=torch.float32, device="cuda")
    x = eng.wrap(x_t.data_ptr(), n)
    out = eng.wrap(out_t.data_ptr(), s_rows)

    def step():
        eng.spmv(PLUS_TIMES_F32, A, x, None, 1.0, 0.0, out)

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        step()
    ev1.record(stream)
    torch.cuda.synchronize()
    fence()
    wall = time.perf_counter() - t0
    dev_ms_per_launch = ev0.elapsed_time(ev1) / args.steps
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())

    if args.dump_outputs or args.full:
        y = out_t.cpu().numpy()[:s_rows]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, y, world, rank)

    # ---- --full: parity of what was just timed (this rank's rows) against the oracle's gold, the CPU baseline
    # and the legs with other value codings.  A plain run stops at the timed steps.
    cpu, parity, bad = None, None, 0
    if args.full:
        cpu, parity, bad = oracle_legs(args, rp, ci, va, s_rp, s_ci, s_va, x_host, y, n, nnz_total, rank, world)

    # ---- transparency leg (N=1): the same matrix without the one-byte value coding, i.e. the layout a
    # matrix with more than 256 distinct values gets; NOT the reported value
    ablation = None
    if args.full and rank == 0 and world == 1 and not args.no_ablation and "values=dict" in A.describe():
        A_raw = eng.upload_csr(s_rows, n, s_rp, s_ci, s_va, value_coding=-1)
        out2_t = torch.zeros_like(out_t)
        out2 = eng.wrap(out2_t.data_ptr(), s_rows)
        for _ in range(3):
            eng.spmv(PLUS_TIMES_F32, A_raw, x, None, 1.0, 0.0, out2)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(20):
            eng.spmv(PLUS_TIMES_F32, A_raw, x, None, 1.0, 0.0, out2)
        e1.record(stream)
        torch.cuda.synchronize()
        raw_ms = e0.elapsed_time(e1) / 20
        raw_traffic, raw_src = measured_traffic(args.workload, A_raw.describe(), world)
        ablation = {"layout": A_raw.describe(), "ms_per_step": round(raw_ms, 6), "traffic": raw_traffic, "traffic_source": raw_src,
                    "frac_of_peak": round(A.algorithmic_bytes(reads_y=False) / (raw_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                    "same_result_bits": bool(torch.equal(out2_t.view(torch.int32), out_t.view(torch.int32))),
                    "note": "value coding off (SH_VALCODE=off): what a matrix with more than 256 distinct values runs at"}
        A_raw.free()

    # ---- third leg (N=1): the same rows and columns with 976 distinct weights -- w + 16 * (k mod 61), integers up to
    # 976 -- i.e. a matrix whose values do not fit the one-byte dictionary: two-byte codes (values=dict16), 4 instead
    # of 6 bytes per entry read by phase 1.  Checked against the oracle's gold on ITS values.
    dict16 = None
    if args.full and rank == 0 and world == 1 and not args.no_ablation and "values=dict" in A.describe():
        from oracle import oracle as O
        va16 = (s_va + np.float32(16) * (np.arange(len(s_va), dtype=np.int64) % 61).astype(np.float32)).astype(np.float32)
        A16 = eng.upload_csr(s_rows, n, s_rp, s_ci, va16)
        out3_t = torch.zeros_like(out_t)
        out3 = eng.wrap(out3_t.data_ptr(), s_rows)
        for _ in range(3):
            eng.spmv(PLUS_TIMES_F32, A16, x, None, 1.0, 0.0, out3)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(20):
            eng.spmv(PLUS_TIMES_F32, A16, x, None, 1.0, 0.0, out3)
        e1.record(stream)
        torch.cuda.synchronize()
        ms16 = e0.elapsed_time(e1) / 20
        y16 = out3_t.cpu().numpy()[:s_rows]
        want16, _ = O.gold_dot_all_cores(s_rp, s_ci, va16, x_host, 1.0, out=np.empty(s_rows, np.float32), threads=usable_host_cores())
        tol16 = 1e-5 * np.maximum(1.0, np.abs(want16.astype(np.float64)))
        off16 = np.nonzero(np.abs(y16.astype(np.float64) - want16.astype(np.float64)) > tol16)[0]
        bad16 = 0
        for r in off16:   # (the same rule as for the headline run: a row whose partial sums pass 2^24 is inexact in the gold itself)
            a, b = int(s_rp[r]), int(s_rp[r + 1])
            terms = x_host[s_ci[a:b]].astype(np.float64) * va16[a:b].astype(np.float64)
            exact = terms.sum()
            if not (np.abs(terms).sum() >= 2 ** 24 and abs(y16[r] - exact) <= 1e-5 * max(1.0, abs(exact)) and abs(y16[r] - exact) <= abs(want16[r] - exact)):
                bad16 += 1
        dict16 = {"layout": A16.describe(), "ms_per_step": round(ms16, 6),
                  "frac_of_peak": round(A16.algorithmic_bytes(reads_y=False) / (ms16 * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                  "mismatches_rel_1e-5": bad16, "rows_excused_like_the_headline_run": int(len(off16) - bad16),
                  "bit_exact_rows": int((y16 == want16).sum()),
                  "note": "weights w + 16 * (k mod 61): 976 distinct values -> two-byte dictionary codes"}
        A16.free()
        bad += bad16

    alg_bytes = A.algorithmic_bytes(reads_y=False)
    achieved = alg_bytes / (dev_ms_per_launch * 1e-3) / 1e9
    layout = A.describe()
    traffic, traffic_src = measured_traffic(args.workload, layout, world) if not (args.rows or args.nnz or args.real_values) else (None, "non-headline run")
    if args.traffic_bytes is not None:
        traffic, traffic_src = args.traffic_bytes, "--traffic-bytes"
    result = {
        "metric": "spmv_gflops", "value": round(2.0 * nnz_total * args.steps / wall / 1e9, 3), "unit": "GFLOP/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 6), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.workload}: {desc}", "rows": n, "nnz": nnz_total, "semiring": "plus-times f32",
                   "alpha": 1.0, "beta": 0.0, "x": "1 + (i mod 7)", "sharding": f"{world} work-balanced contiguous row ranges, x replicated"},
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4),
                     "traffic": traffic, "traffic_source": traffic_src,
                     "kernel": ("sh::spmv_tiled_phase1 + spmv_tiled_phase2s <PlusTimesF32> (one SpMV = these 2 launches)" if A.plan()[0] == "tiled"
                                else "sh::spmv_csr_kernel<PlusTimesF32> (+ spmv_long_fixup)"),
                     "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": round(dev_ms_per_launch, 6),
                     "rank": rank, "rank_nnz": s_nnz},
        "cpu_baseline": cpu,
        # the same matrix with value coding off = what a matrix with more than 256 distinct values runs at;
        # first-class because the headline layout (four-bit codes) owes its stream size to the synthetic weights 1..16
        "frac_raw_values": None if ablation is None else ablation["frac_of_peak"],
        "ms_per_step_raw_values": None if ablation is None else ablation["ms_per_step"],
        "ablation_raw_values": ablation,
        # ... and with a few hundred distinct values: two-byte dictionary codes (the reference's int-narrowed weights,
        # src/sparse_matrix.cpp:107, are small integers but not necessarily <= 256 of them)
        "frac_dict16_values": None if dict16 is None else dict16["frac_of_peak"],
        "ms_per_step_dict16_values": None if dict16 is None else dict16["ms_per_step"],
        "dict16_values": dict16,
        "parity": parity,
        "plan": {"name": A.plan()[0], "streamed_bytes_per_launch": A.plan()[1], "layout": layout, "built_on": A.builder()[0],
                 # (the trial times its own x = 0 / out vectors, four launch pairs at a time: it ranks placements, it does
                 # not predict this loop; the loop's figure stands beside it so that a misprediction shows)
                 "placements_timed_at_upload": dict(zip(("tries", "first_ms", "kept_ms"), A.placement()), loop_avg_launch_ms=round(dev_ms_per_launch, 6))},
        "gen_seconds": round(t_gen, 2), "upload_seconds": round(t_up, 2), "device": eng.device_name,
    }
    if rehearsal:
        result["rehearsal"] = "all ranks shared GPU 0 over gloo: timings are not measurements"
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if bad:
        raise SystemExit(f"parity check failed on rank {rank}: {bad} rows outside 1e-5")


if __name__ == "__main__":
    main()
