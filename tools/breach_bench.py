#!/usr/bin/env python3
"""Depression breaching at 40000 x 40000, HBM resident, in ONE run, on the float32 fractal DEM G(seed=3):

* breach_depressions_dev (rdgpu_breach_d8_dev_f32) beside pf_flowdirs_dev (rdgpu_pf_flowdirs_dev_f32) of the same DEM: host
  clock round calls that end in a synchronise (both iterate the flood's tree from the host), alternating, and the share
  of the breach that is the tree, from the per-kernel times of one profiled call;
* d8_breach_along_dev (`out` alone, `out` + `path`) beside d8_upslope_extreme_dev (the minimum, `extreme` alone) on the
  SAME directions -- the breach's own tree -- with the DEM as levels / values and its local minima as pits: HIP-event time
  per call, alternating lines, medians with min / max as the spread, algorithmic bytes per cell and the fraction of the
  8 TB/s HBM peak at that traffic, then the per-kernel times of one profiled call of each line.

Writes profiles/breach_bench.json (--out).  A failure stops the run: nothing is launched after it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-repeats", type=int, default=2, help="timed calls of each of the two flood lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "breach_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    cells = n * n
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    work = torch.empty_like(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    path = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    res = {"size": n, "launches_per_repeat": args.launches, "repeats": args.repeats, "tree_repeats": args.tree_repeats,
           "hbm_peak_bytes_per_s": HBM_PEAK, "lines": {}, "kernels": {}}

    def profiled(name, fn):
        rd.profile_reset()
        rd.profile_enable(True)
        fn()
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels"][name] = {k: {"ms": round(v[0], 4), "launches": int(v[1])} for k, v in rd.profile_totals().items() if v[1]}

    # ---- the two floods: wall time of whole calls -------------------------------------------------------------------
    def flood_tree():
        rd.pf_flowdirs_dev(Z, -9999.0, dirs)

    def breach():
        work.copy_(Z)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rd.breach_depressions_dev(work, dirs=dirs, path=path)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    wall(flood_tree)                                       # warm-up: workspace growth, code objects
    breach()
    tree_ms, breach_ms = [], []
    for _ in range(args.tree_repeats):                     # alternating
        tree_ms.append(wall(flood_tree))
        breach_ms.append(breach())
    stats = rd.breach_stats()
    for name, ms in (("pf_flowdirs_dev_f32", sorted(tree_ms)), ("breach_d8_dev_f32", sorted(breach_ms))):
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 2), "ms_min": round(ms[0], 2), "ms_max": round(ms[-1], 2)}
        print(name, res["lines"][name], flush=True)
    profiled("breach_d8_dev_f32", breach)
    k = res["kernels"]["breach_d8_dev_f32"]
    carve = sum(v["ms"] for name, v in k.items() if name.startswith("breach."))
    total = sum(v["ms"] for v in k.values())
    res["breach_d8"] = {"stats": stats, "kernel_ms_total": round(total, 2), "kernel_ms_breach_own": round(carve, 3),
                        "tree_share_of_kernel_time": round(1.0 - carve / total, 5) if total else None,
                        "wall_ms_over_pf_flowdirs_wall_ms": round(res["lines"]["breach_d8_dev_f32"]["ms"] /
                                                                  res["lines"]["pf_flowdirs_dev_f32"]["ms"], 3)}
    print("breach_d8", res["breach_d8"], flush=True)

    # ---- the carve beside the upslope minimum on the same directions (the breach's tree, left in `dirs`) ------------
    pits = torch.zeros((n, n), dtype=torch.uint8, device="cuda")
    rows = 2000
    for y0 in range(1, n - 1, rows):                       # local minima of the raw DEM, by row blocks
        y1 = min(n - 1, y0 + rows)
        c = Z[y0:y1, 1:-1]
        lo = torch.full_like(c, float("inf"))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    lo = torch.minimum(lo, Z[y0 + dy:y1 + dy, 1 + dx:n - 1 + dx])
        pits[y0:y1, 1:-1] = (c <= lo).to(torch.uint8)
    del lo, c
    out = work
    torch.cuda.synchronize()

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

    def line(name, fn, bytes_per_cell):
        ms = timed(fn)
        med = ms[len(ms) // 2]
        bps = cells * bytes_per_cell / (med * 1e-3)
        res["lines"][name] = {"ms": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                              "bytes_per_cell": bytes_per_cell, "GB_per_s": round(bps / 1e9, 1),
                              "fraction_of_hbm_peak": round(bps / HBM_PEAK, 4)}
        print(name, res["lines"][name], flush=True)
        profiled(name, fn)
        print(" ", res["kernels"][name], flush=True)

    # bytes per cell, every pass counted: the extreme reads directions three times (3) and the values twice (8), writes 4;
    # the carve reads directions three times (3), the levels three times (12) and the pits twice (2), writes 4 (+ 1)
    products = (("d8_upslope_extreme:min:extreme", lambda: rd.d8_upslope_extreme_dev(dirs, Z, "min", -9999.0, extreme=out), 15),
                ("d8_breach_along:out", lambda: rd.d8_breach_along_dev(dirs, Z, pits, out=out), 21),
                ("d8_breach_along:out+path", lambda: rd.d8_breach_along_dev(dirs, Z, pits, out=out, path=path), 22),
                ("d8_upslope_extreme:min:extreme:again", lambda: rd.d8_upslope_extreme_dev(dirs, Z, "min", -9999.0, extreme=out), 15),
                ("d8_breach_along:out:again", lambda: rd.d8_breach_along_dev(dirs, Z, pits, out=out), 21))
    for name, fn, bpc in products:
        line(name, fn, bpc)
    L = res["lines"]
    ext = min(L["d8_upslope_extreme:min:extreme"]["ms"], L["d8_upslope_extreme:min:extreme:again"]["ms"])
    res["ms_over_upslope_extreme_ms"] = {k: round(v["ms"] / ext, 3) for k, v in L.items() if k.startswith("d8_breach_along")}
    res["pits"] = int(pits.sum().item())
    res["cells_on_a_path"] = int(path.sum().item())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels")}))


if __name__ == "__main__":
    main()
