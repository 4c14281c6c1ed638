#!/usr/bin/env python3
"""Time the batched gradient attribution (utils/sensitivity.py over csrc/pk_attribution.hip) against the loop it replaces, on hrnet_w32
(heatmap head) and hrformer_small (fusion head) with random weights in eval mode, one 256 x 192 crop, all K = 17 joints.

    maps_B       attribution_maps(batch_size=B): ceil(17 / B) x (one forward with grad, one backward to the packed copies, saliency and
                 unpack kernels, Grad-CAM of the backbone's output, heat-map summary); nothing read back
    loop         the reference's procedure with what the library offers without the batched pass: 17 x (batch-1 forward of an input that
                 requires grad, heatmaps[0, k].sum(), torch.autograd.grad to the input, abs().amax(0) in torch); saliency only, no CAM
    no_wgrad_17  maps_17 with the pk_wgrad_bf16 launches skipped: a MEASUREMENT of what the discarded weight gradients cost, not a mode of
                 the library (their results are garbage there, and nothing reads them)

Whole calls, host clock around work that ends in a device synchronise, after one untimed call of every variant; `--rounds` timed calls per
variant, the variants alternating; median and min .. max.  Before anything is timed the results are compared: maps_1 must equal the loop bit
for bit (the same kernels at the same batch); for the larger chunks the relative L2 distance to the loop is reported (0 when no kernel route
changes with the batch).  Prints one JSON line per model.

    python scripts/bench_attribution.py [--models hrnet_w32 hrformer_small] [--batch_sizes 1 4 17] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, K = 256, 192, 17
HEADS = {"hrnet_w32": "heatmap", "hrformer_small": "fusion"}


def reference_loop(model, image):
    """One batch-1 forward and backward per joint -> (K,H,W) saliency on the device."""
    import torch
    out = []
    for k in range(K):
        x = image.clone().requires_grad_(True)
        score = model(x)['heatmaps'][0, k].sum()
        g, = torch.autograd.grad(score, x)
        out.append(g[0].abs().amax(0))
    return torch.stack(out)


def bench(name, args, torch):
    from infantposeestimation_gaussianbias_amd import nnops
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    from infantposeestimation_gaussianbias_amd.utils import attribution_maps
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = PoseEstimator(name, K, False, HEADS[name], True).to(dev).eval()
    image = torch.randn(1, 3, H, W, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, result

    def without_wgrad():
        launch = nnops.call
        nnops.call = lambda entry, *a: None if entry == "pk_wgrad_bf16" else launch(entry, *a)
        try:
            return attribution_maps(model, image, batch_size=K)
        finally:
            nnops.call = launch

    variants = {f"maps_{b}": (lambda b=b: attribution_maps(model, image, batch_size=b)) for b in args.batch_sizes}
    variants["loop"] = lambda: reference_loop(model, image)
    variants[f"no_wgrad_{K}"] = without_wgrad
    first = {k: timed(fn) for k, fn in variants.items()}          # untimed: code objects, weight packing, every batch shape once
    want = first["loop"][1]
    assert bool(want.any()) and bool(torch.isfinite(want).all())
    dist = {}
    for k, (_, res) in first.items():
        if not k.startswith("maps_"):
            continue
        got = res["saliency"]
        assert tuple(got.shape) == (K, H, W) and len(res["layers"]) == 1 and tuple(res["cams"][res["layers"][0]].shape) == (K, H // 4, W // 4)
        dist[k] = float((got.double() - want.double()).norm() / want.double().norm())
        if k == "maps_1":
            assert torch.equal(got, want), "batch_size=1 must repeat the loop's bits"
        assert dist[k] < 0.5, (k, dist[k])                        # sanity only: two bf16 runs of one network, not a tolerance of the library
    assert all(p.grad is None for p in model.parameters())
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn)[0])
    out = {"model": name, "input": [H, W], "joints": K, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "cam_layer": first[f"maps_{args.batch_sizes[0]}"][1]["layers"][0], "saliency_rel_l2_vs_loop": dist,
           "first_call_ms": {k: v[0] for k, v in first.items()}}
    for k, v in t.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_min"], out[f"{k}_ms_max"] = float(np.median(v)), float(min(v)), float(max(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(HEADS), choices=list(HEADS))
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[1, 4, 17])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attribution: no GPU (the kernels have no CPU path)")
    lines = [json.dumps(bench(name, args, torch)) for name in args.models]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
