#!/usr/bin/env python3
"""The depression hierarchy at 40000 x 40000 (f32, G(seed=3), HBM resident) in ONE run from one build: HIP-event time per
call of rdgpu_depression_hierarchy_dev_f32 with labels and with labels = NULL, and of the two yardsticks on the same DEM --
rdgpu_depressions_dev_f32 (the nearest product: the flat inventory of the top-level lakes) and rdgpu_fill_dev_f32.  The
fill works in place, so every timed call of it starts from a fresh copy of the DEM made outside the timed interval.  The
hierarchy's builder runs on the host between two waits for the stream; the events bracket the whole call, the host time
included.  Writes profiles/dephier_bench.json (--out): N, per line the ms (median of the repeats after a warm-up, min / max
as the spread), the ratios to the inventory and to the fill, the hierarchy's counts, then the per-kernel times of one
profiled call of each line ("dephier.builder" is the builder stage: the download of its records and the serial Kruskal),
stamped with the git SHA.  A failure stops the run: nothing is launched after it."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dephier_bench.json"))
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    n = args.size
    Z0 = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z0, seed=3)
    Z = torch.empty_like(Z0)
    labels = torch.empty((n, n), dtype=torch.int32, device="cuda")
    nodes, leaves = (int(v) for v in rd.depression_hierarchy_dev(Z0, None, None).cpu())   # the sizing call
    stats = rd.dephier_stats()
    htable = torch.empty(nodes * rd.DEPHIER_NODE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    lakes = int(rd.depressions_dev(Z0, None, None).item())
    itable = torch.empty((lakes, 5), dtype=torch.float64, device="cuda")
    res = {"git_sha": git_sha(), "size": n, "dtype": "f32", "seed": 3, "repeats": args.repeats, "nodes": nodes, "leaves": leaves,
           "depressions": lakes, "stats": stats, "lines": {}, "kernels_ms": {}}
    print("nodes:", nodes, "leaves:", leaves, "lakes:", lakes, stats, flush=True)

    def fresh():
        Z.copy_(Z0)
        return Z

    lines = (("fill_dev_f32", lambda z: rd.fill_depressions_dev(z), True),
             ("depressions_dev_f32:labels", lambda z: rd.depressions_dev(z, labels, itable), False),
             ("depression_hierarchy_dev_f32:labels", lambda z: rd.depression_hierarchy_dev(z, labels, htable), False),
             ("depression_hierarchy_dev_f32:no_labels", lambda z: rd.depression_hierarchy_dev(z, None, htable), False),
             ("depressions_dev_f32:labels:again", lambda z: rd.depressions_dev(z, labels, itable), False))

    def once(fn, in_place):
        z = fresh() if in_place else Z0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(z)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for name, fn, in_place in lines:
        once(fn, in_place)                                                        # the warm-up
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
    inv = min(L["depressions_dev_f32:labels"]["ms"], L["depressions_dev_f32:labels:again"]["ms"])
    for k in ("depression_hierarchy_dev_f32:labels", "depression_hierarchy_dev_f32:no_labels"):
        res[k + "/depressions"] = round(L[k]["ms"] / inv, 4)
        res[k + "/fill"] = round(L[k]["ms"] / L["fill_dev_f32"]["ms"], 4)
        res[k + ":builder_share"] = round(res["kernels_ms"][k].get("dephier.builder", 0.0) / L[k]["ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in ("lines", "kernels_ms")}))


if __name__ == "__main__":
    main()
