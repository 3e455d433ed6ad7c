#!/usr/bin/env python3
"""p1_timeline.py -- the phase-1 item timeline of one launch, summarised.

Input: the file an -DSH_STATS build of the engine writes with SH_STATS_DUMP=1 SH_STATS_P1_FILE=path
(`make -C sparseharness_amd/csrc stats`; one line per work item: block, kind 0 light / 1 heavy, entries, and the
100 MHz clock at its start, behind the staging of its x tile, and at its end).  Block b runs on XCD b % 8.

Output (one JSON object): per XCD when its last item starts and ends and how much CU time stands idle behind the start
of its last item (no more work can be handed out from then on) -- up to the XCD's own end and up to the end of the
launch; the mean item of each kind; and the cost model a * entries + b * products + c fitted to the means
(c = mean staging; a from the heavy items, which write no P; b from what a light item takes beyond that).

  SH_LIB=sparseharness_amd/variants/stats.so SH_STATS_DUMP=1 SH_STATS_P1_FILE=p1.csv python bench.py --steps 3 --warmup 2
  python tools/p1_timeline.py p1.csv --cus 256 --products 117.5e6 --light 133.9e6
"""
import argparse
import csv
import json

TICK_US = 0.01   # s_memrealtime: 100 MHz


def summarise(path, cus, products_per_entry):
    items = []
    with open(path) as f:
        for r in csv.DictReader(f):
            items.append({k: int(v) for k, v in r.items()})
    if not items:
        raise SystemExit("no items in " + path)
    t0 = min(i["start"] for i in items)
    t_end = max(i["end"] for i in items)
    per = max(1, cus // 8)
    us = lambda ticks: round(ticks * TICK_US, 2)
    xcds = []
    idle_own = idle_launch = 0.0
    for x in range(8):
        mine = [i for i in items if i["block"] % 8 == x]
        if not mine:
            continue
        last_start = max(i["start"] for i in mine)
        own_end = max(i["end"] for i in mine)

        def idle(until):
            busy = sum(max(0, min(i["end"], until) - max(i["start"], last_start)) for i in mine)
            return per * (until - last_start) - busy
        xcds.append({"xcd": x, "items": len(mine), "last_item_starts_us": us(last_start - t0), "last_item_ends_us": us(own_end - t0),
                     "idle_cu_us_behind_last_start_to_own_end": us(idle(own_end)),
                     "idle_cu_us_behind_last_start_to_launch_end": us(idle(t_end))})
        idle_own += idle(own_end)
        idle_launch += idle(t_end)
    span = t_end - t0
    kinds = {}
    for kind, name in ((0, "light"), (1, "heavy")):
        k = [i for i in items if i["kind"] == kind]
        if k:
            kinds[name] = {"items": len(k), "mean_entries": round(sum(i["entries"] for i in k) / len(k), 1),
                           "mean_item_us": us(sum(i["end"] - i["start"] for i in k) / len(k)),
                           "mean_staging_us": us(sum(i["staged"] - i["start"] for i in k) / len(k))}
    out = {"file": path, "cus": cus, "items": len(items), "phase1_span_us": us(span), "per_xcd": xcds,
           "idle_cu_us_to_own_end": us(idle_own), "idle_cu_us_to_launch_end": us(idle_launch),
           "idle_share_of_phase1_cu_time": round(idle_launch / (cus * span), 4), "kinds": kinds}
    if "light" in kinds and "heavy" in kinds:
        c = sum(i["staged"] - i["start"] for i in items) / len(items) * TICK_US * 1e3   # ns
        a = (kinds["heavy"]["mean_item_us"] * 1e3 - c) / kinds["heavy"]["mean_entries"]
        extra = (kinds["light"]["mean_item_us"] * 1e3 - c) / kinds["light"]["mean_entries"] - a
        out["cost_model_ns"] = {"per_item_c": round(c, 1), "per_entry_a": round(a, 4),
                                "light_extra_per_entry": round(extra, 4),
                                "per_product_b": round(extra / products_per_entry, 4) if products_per_entry else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--products", type=float, default=0.0, help="products in P (the layout string's products=)")
    ap.add_argument("--light", type=float, default=0.0, help="light stream entries (the layout string's light=)")
    args = ap.parse_args()
    ppe = args.products / args.light if args.products and args.light else 0.0
    print(json.dumps(summarise(args.file, args.cus, ppe), indent=1))


if __name__ == "__main__":
    main()
