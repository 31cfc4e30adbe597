#!/usr/bin/env python3
"""Are all blocks of the persistent pair pass (k_pairs16) resident at once?  Needs the probe build:

    make -C richdem_amd/csrc probe
    RDGPU_LIB=richdem_amd/librdgpu_probe.so python tools/probes/pairs_residency.py [--size 16000] [--out FILE]

Every block stores wall_clock64() (100 MHz) at entry and at exit.  The grid is sized as blocks per CU x CUs and the tiles
are dealt out over it beforehand, so the blocks are all resident exactly when the LAST one enters before the FIRST one
leaves; a block that had to queue for a slot enters after some other block's exit.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import richdem_amd as rd

    L = rd.lib()
    if not hasattr(L, "rdgpu_probe_pairs_clock"):
        raise SystemExit("not a probe build: set RDGPU_LIB to librdgpu_probe.so (make -C richdem_amd/csrc probe)")
    cap = 8192                                                # blocks the buffer holds: 32 per CU
    clock = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    Z = torch.empty((args.size, args.size), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    W = Z.clone()
    rd.fill_depressions_dev(W)                                # workspace growth, not probed
    W.copy_(Z)
    torch.cuda.synchronize()
    assert L.rdgpu_probe_pairs_clock(ctypes.c_void_p(clock.data_ptr())) == 0
    rd.fill_depressions_dev(W)
    torch.cuda.synchronize()
    assert L.rdgpu_probe_pairs_clock(ctypes.c_void_p(0)) == 0
    c = clock.cpu().numpy().reshape(cap, 2)
    used = c[:, 0] != 0
    n = int(used.sum())
    assert n and used[:n].all(), "the blocks' slots are the first of the buffer"
    ent, ext = c[:n, 0], c[:n, 1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"size": args.size, "blocks": n, "cus": cus, "blocks_per_cu": n / cus,
           "last_entry_minus_first_entry_us": float(ent.max() - ent.min()) / 100.0,
           "first_exit_minus_first_entry_us": float(ext.min() - ent.min()) / 100.0,
           "last_exit_minus_first_entry_us": float(ext.max() - ent.min()) / 100.0,
           "blocks_entering_after_the_first_exit": int((ent > ext.min()).sum()),
           "all_resident": bool(ent.max() < ext.min())}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
