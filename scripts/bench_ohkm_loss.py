#!/usr/bin/env python3
"""Time forward plus backward of the online-hard-keypoint-mining loss (pk_ohkm_loss_fwd / _bwd, csrc/pk_loss.hip) next to the pixel loss
kind 0 (pk_pixel_loss_fwd / _bwd) on the same tensors, by the method of scripts/bench_grad_guard.py: the variants

    pixel       pk_pixel_loss_fwd + pk_pixel_loss_bwd                                  (2 + 1 launches)
    ohkm        pk_ohkm_loss_fwd + pk_ohkm_loss_bwd, topk of K                         (2 + 1 launches)
    ohkm_all    the same with topk = K (every map selected: the pixel loss's arithmetic)

alternate on the same buffers, `--rounds` times; each timing is device events around `--iters` back-to-back forward + backward pairs after
`--warmup` untimed ones, through the C-ABI on preallocated outputs (no allocator, no autograd).  Sizes (B, K, H, W): (64, 17, 64, 48), the
COCO training batch, and (24, 13, 128, 128), the preemie configuration.  Bytes that must move, per pair, N = B K HW floats:
    pixel:  forward reads pred + target (8 N), backward reads both again and writes d_pred (12 N)             -> 20 N bytes
    ohkm:   forward 8 N; backward reads pred + target of the selected maps only and writes every map         -> 8 N + (8 topk / K + 4) N bytes
Prints one JSON line.

    python scripts/bench_ohkm_loss.py [--topk 8] [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_grad_guard import time_steps  # noqa: E402

SIZES = ((64, 17, 64, 48), (24, 13, 128, 128))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topk", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd._lib import call, stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit("bench_ohkm_loss: no GPU (the kernels have no CPU path)")
    torch.manual_seed(0)
    out = {"iters": args.iters, "rounds": args.rounds, "topk": args.topk, "device": torch.cuda.get_device_name(0), "sizes": []}
    for B, K, H, W in SIZES:
        HW, dev = H * W, "cuda"
        pred, target = torch.randn(B, K, H, W, device=dev), torch.rand(B, K, H, W, device=dev)
        weight = (torch.rand(B, K, device=dev) > 0.2).float()
        dp, partial, loss = torch.empty_like(pred), torch.empty(1024, device=dev), torch.empty(1, device=dev)
        per_map, mask = torch.empty(B, K, device=dev), torch.empty(B, K, dtype=torch.uint8, device=dev)
        counts = torch.zeros(K, dtype=torch.int64, device=dev)

        def pixel():
            call("pk_pixel_loss_fwd", pred, target, weight, partial, loss, B, K, HW, 0, stream_ptr())
            call("pk_pixel_loss_bwd", pred, target, weight, None, dp, B, K, HW, 0, stream_ptr())

        def ohkm(topk=args.topk):
            call("pk_ohkm_loss_fwd", pred, target, weight, per_map, mask, loss, counts, B, K, HW, topk, 1.0, stream_ptr())
            call("pk_ohkm_loss_bwd", pred, target, weight, mask, None, dp, B, K, HW, topk, 1.0, stream_ptr())

        variants = {"pixel": pixel, "ohkm": ohkm, "ohkm_all": lambda: ohkm(K)}
        t = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                t[k].append(time_steps(fn, args.warmup, args.iters))
        ohkm()
        torch.cuda.synchronize()
        if int(mask.sum()) != B * args.topk or not bool(torch.isfinite(loss).all()):
            raise SystemExit(f"bench_ohkm_loss: the timed launches did not select {args.topk} maps per sample")
        n = B * K * HW
        nbytes = {"pixel": 20.0 * n, "ohkm": (12.0 + 8.0 * args.topk / K) * n, "ohkm_all": 20.0 * n}
        row = {"shape": [B, K, H, W], "MB_tensor": 4.0 * n / 1e6}
        for k in variants:
            med = float(np.median(t[k]))
            row[f"{k}_us_median"], row[f"{k}_us_min"], row[f"{k}_us_max"] = med, float(min(t[k])), float(max(t[k]))
            row[f"{k}_us_all"] = [round(v, 2) for v in t[k]]
            row[f"{k}_MB_moved"], row[f"{k}_GBps"] = nbytes[k] / 1e6, nbytes[k] / med * 1e-3
        row["ratio_ohkm_over_pixel"] = row["ohkm_us_median"] / row["pixel_us_median"]
        row["ratio_ohkm_all_over_pixel"] = row["ohkm_all_us_median"] / row["pixel_us_median"]
        out["sizes"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
