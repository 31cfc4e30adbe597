#!/usr/bin/env python3
"""Stream reaches at 40000 x 40000, HBM resident, in ONE run: HIP-event time per call of d8_stream_reaches with every cell
a channel and with the channels of d8_channels at thresholds of 10^2 and 10^4 cells (the cases of tools/stream_bench.py),
each with the table alone and with the two label planes as well; in the same run d8_flow_path (to_cell only) with the same
mask -- the comparator: the product contains exactly one such pass plus streaming passes -- and d8_flow_accum (u8 -> f64)
before and after.  Directions: the engine's fill -> flat resolution of G(seed=3).  Writes profiles/stream_reach_bench.json
(--out): per line the ms (median of the repeats, min / max as the spread), N, the per-kernel times and launch counts of
one profiled call, and the ratios to the flow-path call and to the accumulation.  A failure stops the run: nothing is
launched after it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_reach_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    torch.cuda.synchronize()
    del Z
    torch.cuda.empty_cache()
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    masks = {"all_cells": None}
    for thr in (1e2, 1e4):
        masks[f"threshold_{int(thr)}"] = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        rd.d8_channels_dev(area, thr, masks[f"threshold_{int(thr)}"])
    reach = torch.empty((n, n), dtype=torch.int32, device="cuda")
    catchment = torch.empty((n, n), dtype=torch.int32, device="cuda")
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

    def line(name, fn, **extra):
        ms = timed(fn)
        res["lines"][name] = dict({"ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}, **extra)
        print(name, res["lines"][name], flush=True)
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels"][name], flush=True)

    line("d8_flow_accum_f64", lambda: rd.d8_flow_accum_dev(dirs, area))
    for case, mask in masks.items():
        count = int(rd.d8_stream_reaches_dev(dirs, 255, mask).cpu().numpy().view("uint32")[0])     # the sizing call
        table = torch.empty((max(count, 1) * rd.REACH_DTYPE.itemsize,), dtype=torch.uint8, device="cuda")
        line(f"d8_stream_reaches:table:{case}", lambda: rd.d8_stream_reaches_dev(dirs, 255, mask, table=table), reaches=count)
        line(f"d8_stream_reaches:table+planes:{case}",
             lambda: rd.d8_stream_reaches_dev(dirs, 255, mask, reach=reach, catchment=catchment, table=table), reaches=count)
        t = table.cpu().numpy().view(rd.REACH_DTYPE)[:count]
        res["lines"][f"d8_stream_reaches:table+planes:{case}"].update(
            heads=int((t["up"] == 0).sum()), mouths=int((t["down"] == 0).sum()), largest_cells=int(t["cells"].max(initial=0)),
            largest_catchment_cells=int(t["catchment_cells"].max(initial=0)), cells_in_a_catchment=int((catchment != 0).sum().item()))
        # the comparator: the flow-path call with the same mask (without one its stop cells are the outlets)
        line(f"d8_flow_path:to_cell:{case}", lambda: rd.d8_flow_path_dev(dirs, 255, mask, to_cell=reach))
        del table, t
        torch.cuda.empty_cache()
    line("d8_flow_accum_f64:again", lambda: rd.d8_flow_accum_dev(dirs, area))
    L = res["lines"]
    acc = min(L["d8_flow_accum_f64"]["ms"], L["d8_flow_accum_f64:again"]["ms"])
    res["ms_over_flow_path_ms"] = {k: round(v["ms"] / L["d8_flow_path:to_cell:" + k.rsplit(":", 1)[1]]["ms"], 3)
                                   for k, v in L.items() if k.startswith("d8_stream_reaches")}
    res["ms_over_flow_accum_ms"] = {k: round(v["ms"] / acc, 3) for k, v in L.items() if k.startswith(("d8_stream_reaches", "d8_flow_path"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
