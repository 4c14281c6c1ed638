#!/usr/bin/env python3
"""Time the feature-sheet and heat-map-quality entries (csrc/pk_panels.hip through hipops) against the obvious on-device torch
composition, at the sizes of the workload: the 96 x 72 quarter-resolution maps of a 384 x 288 crop, 17 joints, batches of 32.

    feature_sheet   16 channels of a (1,96,72,C) bf16 map at zoom 4, four per row, pad 2: pk_gather_planes + pk_plane_sheet (three
                    launches) against index, amin / amax, the index rule, a LUT gather, repeat_interleave and one slice copy per tile
    quality_sheet   the 17 x 3 target / prediction / difference sheet of (17,96,72) maps at zoom 1: torch.cat + pk_plane_sheet against
                    the same composition over 51 tiles
    quality         pk_heatmap_quality at M = 32 x 17 maps of 96 x 72 against (p - g).pow(2).sum, amax, argmax, the centred second pass
                    and the two half-maximum counts in torch (float64 sums, as the kernel's)

Whole calls on the current stream, `--iters` calls between two device synchronises under a host clock, after one untimed window of every
variant; `--rounds` timed windows per variant, the variants alternating; median and min .. max of the time per call in microseconds.
Before anything is timed the results are compared: the number of sheet pixels on which the torch composition and the kernel differ is
reported (the kernel's arithmetic is pinned, torch's is whatever its kernels do), and the sums must agree to 1e-9 relative.  Nothing is
copied to the host inside a timed window.  Prints one JSON line.

    python scripts/bench_panels.py [--channels 64] [--iters 500] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, K, B = 96, 72, 17, 32


def torch_tiles_sheet(torch, tiles, luts, ramps, cols, zoom, pad):
    """tiles (T,h,w) fp32 -> (SH,SW,3) uint8: every tile scaled to its own range, looked up, zoomed, copied into a white sheet."""
    T, h, w = tiles.shape
    lo, hi = tiles.amin(dim=(1, 2), keepdim=True), tiles.amax(dim=(1, 2), keepdim=True)
    idx = (255.0 * ((tiles - lo) / ((hi - lo) + 1e-8))).floor().clamp(0, 255).long()
    rgb = luts[ramps[:, None, None], idx]                                        # (T,h,w,3)
    rgb = rgb.repeat_interleave(zoom, dim=1).repeat_interleave(zoom, dim=2)
    rows = -(-T // cols)
    sheet = torch.full((pad + rows * (h * zoom + pad), pad + cols * (w * zoom + pad), 3), 255, dtype=torch.uint8, device=tiles.device)
    for t in range(T):
        y0, x0 = pad + (t // cols) * (h * zoom + pad), pad + (t % cols) * (w * zoom + pad)
        sheet[y0:y0 + h * zoom, x0:x0 + w * zoom] = rgb[t]
    return sheet


def torch_quality(torch, p, g):
    """(M,h,w) fp32 x2 -> (M,13) float64: the columns of pk_heatmap_quality that have a one-line torch form (0-4, 7, 10-14 and the two
    flat peak indices), for finite maps."""
    M, h, w = p.shape
    pd, gd = p.double().reshape(M, -1), g.double().reshape(M, -1)
    d = pd - gd
    mp, ip = p.reshape(M, -1).max(dim=1)
    mg, ig = g.reshape(M, -1).max(dim=1)
    cp, cg = pd - pd.mean(dim=1, keepdim=True), gd - gd.mean(dim=1, keepdim=True)
    ok = ((mp > 0) & (mg > 0))[:, None]
    in_p, in_g = ok & (p.reshape(M, -1) >= 0.5 * mp[:, None]), ok & (g.reshape(M, -1) >= 0.5 * mg[:, None])
    return torch.stack([pd.sum(1), gd.sum(1), d.pow(2).sum(1), d.abs().amax(1), mp.double(), ip.double(), mg.double(), ig.double(),
                        (cp * cg).sum(1), cp.pow(2).sum(1), cg.pow(2).sum(1), (in_p & in_g).sum(1).double(), (in_p | in_g).sum(1).double()], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64, help="channels of the tapped map (a multiple of 8)")
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_panels: no GPU (the kernels have no CPU path)")
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd.utils.feature_maps import heatmap_quality_sheet
    from infantposeestimation_gaussianbias_amd.utils.visualization import colour_ramp
    dev = torch.device("cuda")
    torch.manual_seed(0)
    C = args.channels
    fmap = torch.randn(1, H, W, C, device=dev).to(torch.bfloat16)
    chans = torch.arange(16, dtype=torch.int32, device=dev)
    tiles16 = torch.tensor([[i, -1, 0] for i in range(16)], dtype=torch.int32, device=dev)
    luts = torch.from_numpy(np.stack([colour_ramp("sequential"), colour_ramp("hot"), colour_ramp("diverging")])).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    cx, cy = torch.rand(B * K, 1, 1, device=dev) * (W - 1), torch.rand(B * K, 1, 1, device=dev) * (H - 1)
    gt = torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 8.0)
    pred = (0.8 * torch.exp(-((xx - cx - 1.3) ** 2 + (yy - cy + 0.7) ** 2) / 8.0) + 0.01 * torch.randn(B * K, H, W, device=dev)).contiguous()
    p17, g17 = pred[:K].contiguous(), gt[:K].contiguous()
    ramps16 = torch.zeros(16, dtype=torch.long, device=dev)
    ramps51 = torch.tensor([1, 1, 2] * K, dtype=torch.long, device=dev)

    def kernel_feature_sheet():
        return hipops.plane_sheet(hipops.gather_planes(fmap, chans, 0, C), tiles16, luts, cols=4, zoom=4, pad=2)[0]

    def torch_feature_sheet():
        return torch_tiles_sheet(torch, fmap[0, :, :, :16].permute(2, 0, 1).float(), luts, ramps16, 4, 4, 2)

    def kernel_quality_sheet():
        return heatmap_quality_sheet(p17, g17, zoom=1, pad=2)[0]

    def torch_quality_sheet():
        tiles = torch.stack([g17, p17, (p17 - g17).abs()], dim=1).reshape(3 * K, H, W)
        return torch_tiles_sheet(torch, tiles, luts, ramps51, 3, 1, 2)

    variants = {"feature_sheet": (kernel_feature_sheet, torch_feature_sheet), "quality_sheet": (kernel_quality_sheet, torch_quality_sheet),
                "quality": (lambda: hipops.heatmap_quality(pred, gt), lambda: torch_quality(torch, pred, gt))}

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.iters

    out = {"device": torch.cuda.get_device_name(0), "map": [H, W], "channels": C, "iters": args.iters, "rounds": args.rounds}
    for name in ("feature_sheet", "quality_sheet"):
        a, b = variants[name][0](), variants[name][1]()
        assert a.shape == b.shape and a.dtype == b.dtype == torch.uint8, (name, a.shape, b.shape)
        out[f"{name}_size"] = list(a.shape[:2])
        out[f"{name}_pixels_differ"] = int((a != b).any(dim=2).sum())
        assert out[f"{name}_pixels_differ"] <= a.shape[0] * a.shape[1] // 20, (name, out[f"{name}_pixels_differ"])      # sanity, not a tolerance
    rec, ref = variants["quality"][0](), variants["quality"][1]()
    flat = lambda x, y: y * W + x                                               # noqa: E731
    got = torch.stack([rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], flat(rec[:, 5], rec[:, 6]), rec[:, 7], flat(rec[:, 8], rec[:, 9]),
                       rec[:, 10], rec[:, 11], rec[:, 12], rec[:, 13], rec[:, 14]], dim=1)
    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
    out["quality_max_rel_diff_vs_torch"] = rel
    assert rel <= 1e-9, rel
    for fns in variants.values():                                               # untimed: code objects, allocator, every shape once
        for fn in fns:
            window(fn)
    t = {(name, side): [] for name in variants for side in ("kernel", "torch")}
    for _ in range(args.rounds):
        for name, fns in variants.items():
            for side, fn in zip(("kernel", "torch"), fns):
                t[name, side].append(window(fn))
    for (name, side), v in t.items():
        out[f"{name}_{side}_us_median"], out[f"{name}_{side}_us_min"], out[f"{name}_{side}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
