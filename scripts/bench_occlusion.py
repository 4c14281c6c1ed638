#!/usr/bin/env python3
"""Time the occlusion sensitivity sweep (utils/sensitivity.py over csrc/pk_occlusion.hip) against the reference's procedure on the same
model: hrnet_w32 (heatmap head, random weights) in eval mode, one 256 x 192 crop, patch 16, stride 8 -> 30 x 22 = 660 occluded copies.

    sweep_B      occlusion_sensitivity_maps(batch_size=B): ceil(660 / B) + 1 forwards, three kernels around them, the maps of all 17 joints
    loop         what analysis/advanced_analysis.py:387-427 does, with what the library offered before the sweep: 660 batch-1 forwards on
                 torch-sliced clones of the image, `.sum().item()` after each, the map of ONE joint filled on the host

Whole calls, host clock around work that ends in a device synchronise (the loop synchronises 661 times by itself), after one untimed call
of every variant; `--rounds` timed calls per variant, the variants alternating; median and min .. max.  Before anything is timed the
sweep's map of the joint is compared with the loop's: the loop sums in float32 in torch's order, so they agree to float32 summation error,
not bit for bit.  Prints one JSON line.

    python scripts/bench_occlusion.py [--batch_sizes 16 32 64 128 256 660] [--rounds 3] [--joint 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, PATCH, STRIDE, K = 256, 192, 16, 8, 17


def reference_loop(model, image, joint, patch, stride):
    """The reference's procedure, restated: one forward and one host read per patch position, one joint."""
    import torch
    h, w = image.shape[2:]
    out = np.zeros((h, w))
    with torch.no_grad():
        base = model(image)['heatmaps'][0, joint].sum().item()
        for i in range(0, h - patch, stride):
            for j in range(0, w - patch, stride):
                occluded = image.clone()
                occluded[:, :, i:i + patch, j:j + patch] = 0
                out[i:i + patch, j:j + patch] = base - model(occluded)['heatmaps'][0, joint].sum().item()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[16, 32, 64, 128, 256, 660])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--joint", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    from infantposeestimation_gaussianbias_amd.utils import occlusion_sensitivity_maps
    if not torch.cuda.is_available():
        raise SystemExit("bench_occlusion: no GPU (the kernels have no CPU path)")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = PoseEstimator("hrnet_w32", K, False, "heatmap", True).to(dev).eval()
    image = torch.randn(1, 3, H, W, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, result

    variants = {f"sweep_{b}": (lambda b=b: occlusion_sensitivity_maps(model, image, PATCH, STRIDE, batch_size=b)) for b in args.batch_sizes}
    variants["loop"] = lambda: reference_loop(model, image, args.joint, PATCH, STRIDE)
    first = {k: timed(fn) for k, fn in variants.items()}          # untimed: code objects, weight packing, every batch shape once
    want = first["loop"][1]
    with torch.no_grad():
        mass = float(model(image)['heatmaps'][0, args.joint].float().abs().sum())
    bound = 2 * 2.0 ** -24 * (H // 4) * (W // 4) * mass                      # two float32 sums of h w terms each, against exact
    diffs = {}
    for k, (_, res) in first.items():
        if k == "loop":
            continue
        assert res["grid"] == (30, 22)
        got = res["maps"][args.joint].cpu().numpy()
        diffs[k] = float(np.abs(got - want).max())
        assert diffs[k] <= bound, (k, diffs[k], bound)
        assert torch.equal(res["maps"], first[f"sweep_{args.batch_sizes[0]}"][1]["maps"]), k      # the chunk size changes no bit
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn)[0])
    out = {"model": "hrnet_w32", "input": [H, W], "patch": PATCH, "stride": STRIDE, "copies": 660, "joints_sweep": K, "joints_loop": 1,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "max_abs_diff_vs_loop": max(diffs.values()), "diff_bound": bound, "joint_abs_sum": mass,
           "first_call_ms": {k: v[0] for k, v in first.items()}}
    for k, v in t.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_min"], out[f"{k}_ms_max"] = float(np.median(v)), float(min(v)), float(max(v))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
