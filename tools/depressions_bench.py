#!/usr/bin/env python3
"""The depression inventory at 40000 x 40000 (f32, G(seed=3), HBM resident) in ONE run from one build: HIP-event time per
call of rdgpu_depressions_dev_f32 with labels and with labels = NULL, and of the two yardsticks on the same DEM --
rdgpu_fill_dev_f32 and rdgpu_fill_max_dep_dev_f32 (the same local phase and pocket union as the inventory).  The fills
work in place, so every timed call of them starts from a fresh copy of the DEM made outside the timed interval.  Writes
profiles/depressions_bench.json (--out): N, per line the ms (median of the repeats, min / max as the spread), the ratios
to each yardstick, then the per-kernel times of one profiled call of each line, stamped with the git SHA.  A failure
stops the run: nothing is launched after it."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def git_sha():
    if os.environ.get("RDGPU_GIT_SHA"):
        return os.environ["RDGPU_GIT_SHA"]
    try:
        with open(os.path.join(ROOT, ".gitsha")) as f:
            return f.read().strip()
    except OSError:
        pass
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-dep", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depressions_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z0 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z0, seed=3)
    Z = torch.empty_like(Z0)
    labels = torch.empty((n, n), dtype=torch.int32, device="cuda")
    count = int(rd.depressions_dev(Z0, None, None).item())   # the sizing call
    table = torch.empty((count, 5), dtype=torch.float64, device="cuda")
    res = {"git_sha": git_sha(), "size": n, "dtype": "f32", "seed": 3, "repeats": args.repeats, "max_dep_size": args.max_dep,
           "depressions": count, "lines": {}, "kernels_ms": {}}
    print("depressions:", count, flush=True)

    def fresh():
        Z.copy_(Z0)
        return Z

    lines = (("fill_dev_f32", lambda z: rd.fill_depressions_dev(z), True),
             ("fill_max_dep_dev_f32", lambda z: rd.fill_max_dep_dev(z, args.max_dep), True),
             ("depressions_dev_f32:labels", lambda z: rd.depressions_dev(z, labels, table), False),
             ("depressions_dev_f32:no_labels", lambda z: rd.depressions_dev(z, None, table), False),
             ("fill_max_dep_dev_f32:again", lambda z: rd.fill_max_dep_dev(z, args.max_dep), True))

    def once(fn, in_place):
        z = fresh() if in_place else Z0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(z)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for name, fn, in_place in lines:
        for _ in range(2):
            once(fn, in_place)
        ms = sorted(once(fn, in_place) for _ in range(args.repeats))
        res["lines"][name] = {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3)}
        print(name, res["lines"][name], flush=True)
        z = fresh() if in_place else Z0
        torch.cuda.synchronize()
        rd.profile_reset()
        rd.profile_enable(True)
        fn(z)
        rd.profile_collect()
        rd.profile_enable(False)
        res["kernels_ms"][name] = {k: round(v[0], 4) for k, v in rd.profile_totals().items() if v[1]}
        print(" ", res["kernels_ms"][name], flush=True)
    L = res["lines"]
    md = min(L["fill_max_dep_dev_f32"]["ms"], L["fill_max_dep_dev_f32:again"]["ms"])
    for k in ("depressions_dev_f32:labels", "depressions_dev_f32:no_labels"):
        res[k + "/fill_max_dep"] = round(L[k]["ms"] / md, 4)
        res[k + "/fill"] = round(L[k]["ms"] / L["fill_dev_f32"]["ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels_ms")}))


if __name__ == "__main__":
    main()
