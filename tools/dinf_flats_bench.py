#!/usr/bin/env python3
"""D-infinity accumulation across flats at 40000 x 40000, HBM resident, in ONE run on G(seed=3) after the fill:
  fa_tarboton_flats_dev                          the drainable flats pass flow on, the DEM is not altered
  fa_tarboton_dev                                the plain accumulation on the same filled DEM (it stops at every lake),
                                                 measured before and after the others: the yardstick and its spread
  resolve_flats_epsilon_dev + fa_tarboton_dev    on a copy: the route there was before (it alters the DEM)
  d8_flow_directions_dev(flats=True)             the D8 branch's flat resolution (directions only), for scale
A call synchronises its stream where it reads counts back, so a call is timed with the host clock around it, ending in a
device synchronise; per line the median of the repeats after one warm-up call, min / max as the spread.  Writes
profiles/dinf_flats_bench.json (--out): the lines, their ratios to fa_tarboton_dev, the four counts of
dinf_flats_stats, and the per-kernel times of one profiled fa_tarboton_flats_dev call (a run of its own, after the timed
ones).  A failure stops the run."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dinf_flats_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    acc = torch.empty((n, n), dtype=torch.float64, device="cuda")
    Zc = torch.empty_like(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"size": n, "repeats": args.repeats, "lines": {}, "kernels": {}}

    def fa_flats():
        acc.fill_(1.0)
        rd.fa_tarboton_flats_dev(Z, -9999.0, acc)

    def fa_plain():
        acc.fill_(1.0)
        rd.fa_tarboton_dev(Z, -9999.0, acc)

    def fa_epsilon():
        Zc.copy_(Z)
        rd.resolve_flats_epsilon_dev(Zc, -9999.0)
        acc.fill_(1.0)
        rd.fa_tarboton_dev(Zc, -9999.0, acc)

    def line(name, fn, after=None):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}
        if after:
            res["lines"][name].update(after())
        print(name, res["lines"][name], flush=True)

    def reached():
        return {"work_list_launches": rd.flow_accumulation_rounds(), "max_accumulation": float(acc.max().item())}

    line("fa_tarboton_dev", fa_plain, reached)
    line("fa_tarboton_flats_dev", fa_flats, reached)
    res["stats"] = rd.dinf_flats_stats()
    line("resolve_flats_epsilon_dev+fa_tarboton_dev", fa_epsilon, reached)
    line("d8_flow_directions_dev:flats", lambda: rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True))
    line("fa_tarboton_dev:again", fa_plain, reached)
    L = res["lines"]
    yard = min(L["fa_tarboton_dev"]["ms"], L["fa_tarboton_dev:again"]["ms"])
    res["ms_over_fa_tarboton_dev_ms"] = {k: round(v["ms"] / yard, 3) for k, v in L.items() if not k.startswith("fa_tarboton_dev")}
    res["flats_ms_over_epsilon_route_ms"] = round(L["fa_tarboton_flats_dev"]["ms"] / L["resolve_flats_epsilon_dev+fa_tarboton_dev"]["ms"], 3)
    rd.profile_reset()
    rd.profile_enable(True)
    fa_flats()
    rd.profile_collect()
    rd.profile_enable(False)
    res["kernels"]["fa_tarboton_flats_dev"] = {k: {"ms": round(v[0], 3), "launches": int(v[1])}
                                               for k, v in rd.profile_totals().items() if v[1]}
    print(" ", res["kernels"]["fa_tarboton_flats_dev"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
