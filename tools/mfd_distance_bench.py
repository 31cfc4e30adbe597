#!/usr/bin/env python3
"""Distance and drop down to the channels over D-infinity proportions at 40000 x 40000, HBM resident, in ONE run:
dinf_distance_down_dev for dist alone, drop alone and both (stat ave, strict), and fa_tarboton_dev -- the accumulation
over the same graph, which also visits every cell once -- on the same DEM as the yardstick, measured before and after.
The DEM is G(seed=3) after the fill and resolve_flats_epsilon_dev: every cell drains.  Channels: >= 100 cells of
D-infinity accumulation.  A call synchronises its stream once per work-list launch, so a call is timed with the host
clock around it, ending in a device synchronise; per line the median of the repeats after one warm-up call, min / max as
the spread.  Writes profiles/mfd_distance_bench.json (--out): the lines, the work-list launches of each, the ratio of each
distance line to fa_tarboton_dev, the shares of resolved cells, and the per-kernel times of one profiled call of the
"both" line and of the accumulation (a run of their own, after the timed ones).  A failure stops the run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfd_distance_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    rd.resolve_flats_epsilon_dev(Z, -9999.0)
    acc = torch.empty((n, n), dtype=torch.float64, device="cuda")
    acc.fill_(1.0)
    rd.fa_tarboton_dev(Z, -9999.0, acc)
    chan = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_channels_dev(acc, args.threshold, chan)
    dist = torch.empty((n, n), dtype=torch.float64, device="cuda")
    drop = torch.empty((n, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = {"size": n, "repeats": args.repeats, "channel_threshold": args.threshold,
           "channel_cells": int(chan.count_nonzero().item()), "lines": {}, "kernels": {}}

    def fa():
        acc.fill_(1.0)
        rd.fa_tarboton_dev(Z, -9999.0, acc)

    def line(name, fn, rounds):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                              "work_list_launches": rounds()}
        print(name, res["lines"][name], flush=True)

    lines = (("fa_tarboton_dev", fa, rd.flow_accumulation_rounds),
             ("dinf_distance_down_dev:dist", lambda: rd.dinf_distance_down_dev(Z, -9999.0, chan, "ave", True, dist=dist),
              rd.mfd_distance_rounds),
             ("dinf_distance_down_dev:drop", lambda: rd.dinf_distance_down_dev(Z, -9999.0, chan, "ave", True, drop=drop),
              rd.mfd_distance_rounds),
             ("dinf_distance_down_dev:dist+drop",
              lambda: rd.dinf_distance_down_dev(Z, -9999.0, chan, "ave", True, dist=dist, drop=drop), rd.mfd_distance_rounds),
             ("fa_tarboton_dev:again", fa, rd.flow_accumulation_rounds))
    for name, fn, rounds in lines:
        line(name, fn, rounds)
    L = res["lines"]
    res["cells_resolved"] = int((dist != -1.0).sum().item())
    res["fraction_resolved"] = round(res["cells_resolved"] / (n * n), 4)
    yard = min(L["fa_tarboton_dev"]["ms"], L["fa_tarboton_dev:again"]["ms"])
    res["ms_over_fa_tarboton_dev_ms"] = {k: round(v["ms"] / yard, 3) for k, v in L.items() if k.startswith("dinf_")}
    for name, fn in (("dinf_distance_down_dev:dist+drop", lines[3][1]), ("fa_tarboton_dev", fa)):
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 3), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", name, res["kernels"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
