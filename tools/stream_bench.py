#!/usr/bin/env python3
"""Stream order at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_stream_order with every cell a
channel and with the channels of d8_channels at thresholds of 10^2 and 10^4 cells, with d8_flow_accum (u8 -> f64) on the
same directions as the yardstick, before and after.  Directions: the engine's fill -> flat resolution of G(seed=3).
Writes profiles/stream_bench.json (--out): per line the ms (median of the repeats, min / max as the spread), the
per-kernel times and launch counts of one profiled call, the levels / node rounds / launches enqueued, the levels that
ran (the largest order), and the ratio to the accumulation.  --check N: one N x N raster against the Python model
(tests/stream_model.py), recorded, not asserted elsewhere.  A failure stops the run: nothing is launched after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dirs_of(rd, torch, n, seed):
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=seed)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    torch.cuda.synchronize()
    return dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import richdem_amd as rd

    n = args.size
    dirs = dirs_of(rd, torch, n, 3)
    torch.cuda.empty_cache()
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    chans = {}
    for thr in (1e2, 1e4):
        chans[thr] = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        rd.d8_channels_dev(area, thr, chans[thr])
    order = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    res = {"size": n, "launches_per_repeat": args.launches, "repeats": args.repeats, "lines": {}, "kernels": {}}

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / args.launches)
        return sorted(ms)

    def line(name, fn, is_order):
        ms = timed(fn)
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
        if is_order:
            finite = order[order != 255]
            res["lines"][name].update(rd.d8_stream_order_stats(), largest_order=int(finite.max().item()),
                                      channel_cells=int((order != 0).sum().item()), loop_cells=int((order == 255).sum().item()))
        print(name, res["lines"][name], flush=True)
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels"][name], flush=True)

    line("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area), False)
    line("d8_stream_order:all_cells", lambda: rd.d8_stream_order_dev(dirs, order), True)
    for thr, c in chans.items():
        line(f"d8_stream_order:threshold_{int(thr)}", lambda c=c: rd.d8_stream_order_dev(dirs, order, 255, c), True)
    line("d8_channels", lambda: rd.d8_channels_dev(area, 1e2, chans[1e2]), False)
    line("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area), False)
    L = res["lines"]
    acc = min(L["d8_flow_accum_f64"]["ms"], L["d8_flow_accum_f64:again"]["ms"])
    res["stream_order_ms_over_flow_accum_ms"] = {k: round(v["ms"] / acc, 3) for k, v in L.items() if k.startswith("d8_stream_order")}
    if args.check:
        import stream_model as sm

        del area, chans, order
        torch.cuda.empty_cache()
        m = args.check
        d = dirs_of(rd, torch, m, 5)
        a = torch.empty((m, m), dtype=torch.float64, device="cuda")
        rd.d8_flow_accum_dev(d, a)
        c = torch.empty((m, m), dtype=torch.uint8, device="cuda")
        rd.d8_channels_dev(a, 50.0, c)
        o = torch.empty((m, m), dtype=torch.uint8, device="cuda")
        rd.d8_stream_order_dev(d, o, 255, c)
        torch.cuda.synchronize()
        exp = sm.stream_order(d.cpu().numpy(), 255, c.cpu().numpy())
        got = o.cpu().numpy()
        res["model_check"] = {"size": m, "threshold": 50.0, "channel_cells": int((exp != 0).sum()), "largest_order": int(exp.max()),
                              "cells_differing": int((got != exp).sum())}
        print("model check", res["model_check"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))
    return 0 if res.get("model_check", {}).get("cells_differing", 0) == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
