#!/usr/bin/env python3
"""Reverse accumulation and upslope dependence over D-infinity proportions at 40000 x 40000, HBM resident, in ONE run:
dinf_reverse_accum_dev for the dependence on the channels (>= 100 cells of D-infinity accumulation), for racc alone and for
racc + wmax over a random weight raster, with the two neighbouring engines as yardsticks on the same DEM, their lines
alternating with the new ones: fa_tarboton_dev -- the accumulation over the same graph, the other way -- and
dinf_distance_down_dev with dist alone (ave, strict, the same channel mask: the same graph in the same direction with one
value plane).  The DEM is G(seed=3) after the fill and resolve_flats_epsilon_dev: every cell drains.  A call synchronises its
stream once per work-list launch, so a call is timed with the host clock around it, ending in a device synchronise; per
line the median of the repeats after one warm-up call, min / max as the spread.  Writes profiles/mfd_reverse_bench.json
(--out): the lines, the work-list launches of each, the ratio of each new line to the two yardsticks (the lower median of
each yardstick's lines), the share of decided cells, the racc line again under other settings of
RDGPU_MFD_DISTANCE_STACK_BELOW (--sweep), and the per-kernel times of one profiled call of each new line (runs of their own,
after the timed ones).  A failure stops the run."""
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
    ap.add_argument("--sweep", default="0,16384,262144", help="settings of RDGPU_MFD_DISTANCE_STACK_BELOW for the racc line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfd_reverse_bench.json"))
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
    torch.manual_seed(3)
    wts = torch.rand((n, n), dtype=torch.float64, device="cuda")
    racc = torch.empty((n, n), dtype=torch.float64, device="cuda")
    wmax = torch.empty((n, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = {"size": n, "repeats": args.repeats, "channel_threshold": args.threshold,
           "channel_cells": int(chan.sum(dtype=torch.int64).item()), "lines": {}, "kernels": {}}

    def fa():
        acc.fill_(1.0)
        rd.fa_tarboton_dev(Z, -9999.0, acc)

    def down():
        rd.dinf_distance_down_dev(Z, -9999.0, chan, "ave", True, dist=racc)

    def dep():
        rd.dinf_reverse_accum_dev(Z, -9999.0, None, chan, racc=racc)

    def rev():
        rd.dinf_reverse_accum_dev(Z, -9999.0, wts, None, racc=racc)

    def both():
        rd.dinf_reverse_accum_dev(Z, -9999.0, wts, None, racc=racc, wmax=wmax)

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

    FA, DOWN, REV = "fa_tarboton_dev", "dinf_distance_down_dev:dist", "dinf_reverse_accum_dev"
    new = {REV + ":dependence": dep, REV + ":racc": rev, REV + ":racc+wmax": both}
    lines = ((FA + "#1", fa, rd.flow_accumulation_rounds),
             (REV + ":dependence", dep, rd.mfd_distance_rounds),
             (DOWN + "#1", down, rd.mfd_distance_rounds),
             (REV + ":racc", rev, rd.mfd_distance_rounds),
             (FA + "#2", fa, rd.flow_accumulation_rounds),
             (REV + ":racc+wmax", both, rd.mfd_distance_rounds),
             (DOWN + "#2", down, rd.mfd_distance_rounds),
             (FA + "#3", fa, rd.flow_accumulation_rounds))
    for name, fn, rounds in lines:
        line(name, fn, rounds)
        if name in new:
            res["lines"][name]["fraction_decided"] = round(int((racc != -1.0).sum().item()) / (n * n), 4)
        if name == REV + ":dependence":
            res["lines"][name]["fraction_strictly_between_0_and_1"] = round(int(((racc > 0.0) & (racc < 1.0)).sum().item()) / (n * n), 4)
    L = res["lines"]
    yard_fa = min(v["ms"] for k, v in L.items() if k.startswith(FA))
    yard_down = min(v["ms"] for k, v in L.items() if k.startswith(DOWN))
    res["ms_over_fa_tarboton_dev_ms"] = {k: round(v["ms"] / yard_fa, 3) for k, v in L.items() if k in new}
    res["ms_over_dinf_distance_down_dev_dist_ms"] = {k: round(v["ms"] / yard_down, 3) for k, v in L.items() if k in new}
    # the racc line under other settings of the switch between the two work-list kernels (the default is unset)
    env = "RDGPU_MFD_DISTANCE_STACK_BELOW"
    keep = os.environ.get(env)
    for sb in [s for s in args.sweep.split(",") if s]:
        os.environ[env] = sb
        line(f"{REV}:racc:{env}={sb}", rev, rd.mfd_distance_rounds)
    if keep is None:
        os.environ.pop(env, None)
    else:
        os.environ[env] = keep
    for name, fn in list(new.items()) + [(DOWN, down)]:
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
