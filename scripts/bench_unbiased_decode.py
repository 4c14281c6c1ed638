#!/usr/bin/env python3
"""Time the unbiased (DARK) decode against the quarter-shift decode on the device: `hipops.unbiased_decode(kernel=11)` and
`hipops.argmax_decode(mode=1)` (pk_unbiased_decode / pk_argmax_decode, csrc/pk_decode.hip) on the same heatmaps, inputs already on the
device, at the COCO shape (64, 17, 64, 48) and the infant shape (64, 13, 128, 128).  Both kernels read every map once; the unbiased one
then blurs a (kernel + 4) x 5 patch per map.  Each figure is a host clock around `--inner` back-to-back calls that ends in a synchronise,
divided by `--inner` (one call is a few microseconds: a single call would time the clock); the two decodes alternate inside every repeat.
Warm-up first, then `--repeats` repeats.  The maps are those of the tests' generator (tests/unbiased_np.py), and the coordinates of the
two decodes are compared with the true centres.  Prints one JSON line.

    python scripts/bench_unbiased_decode.py [--repeats 30] [--inner 200] [--kernel 11] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unbiased_np as unp  # noqa: E402

SHAPES = ((64, 17, 64, 48), (64, 13, 128, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--kernel", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd import hipops
    if not torch.cuda.is_available():
        raise SystemExit("bench_unbiased_decode: no GPU (the kernels have no CPU path)")
    dev = torch.device("cuda")
    out = {"repeats": args.repeats, "inner": args.inner, "kernel": args.kernel, "device": torch.cuda.get_device_name(0)}
    for B, K, H, W in SHAPES:
        maps, centres = unp.make_maps(B * K, H, W, seed=0)
        hm = torch.from_numpy(maps).to(dev).view(B, K, H, W)
        runs = {"argmax_mode1": lambda: hipops.argmax_decode(hm, 1), "unbiased": lambda: hipops.unbiased_decode(hm, args.kernel)}
        for fn in runs.values():                                  # warm-up: code objects, allocator
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in runs}
        for _ in range(args.repeats):
            for name, fn in runs.items():
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.inner)
        shift, unb = runs["argmax_mode1"]()[2], runs["unbiased"]()
        res = {"map_bytes": int(maps.nbytes)}
        for name, ts in times.items():
            res[name] = {"us_median": 1e6 * float(np.median(ts)), "us_min": 1e6 * float(np.min(ts)), "us_max": 1e6 * float(np.max(ts))}
        res["ratio_unbiased_over_mode1"] = res["unbiased"]["us_median"] / res["argmax_mode1"]["us_median"]
        res["steps_taken"] = int(unb[3].sum())
        res["mean_error_px"] = {"argmax_mode1": unp.mean_error(shift.cpu().numpy().reshape(-1, 2), centres),
                                "unbiased": unp.mean_error(unb[2].cpu().numpy().reshape(-1, 2), centres)}
        out[f"{B}x{K}x{H}x{W}"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
