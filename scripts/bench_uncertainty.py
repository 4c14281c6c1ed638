#!/usr/bin/env python3
"""Time the stochastic-depth ensemble (utils/uncertainty.py over csrc/pk_ensemble.hip) against the reference's procedure restated on this
library: hrformer_small (fusion head, random weights) in eval mode, one 256 x 192 crop, S = 30 members.

    ensemble_B   mc_uncertainty(batch_size=B): ceil(30 / B) forwards under nnops.stochastic_depth, then pk_ensemble_moments, three
                 pk_heatmap_summary and two pk_ensemble_points launches; maps and per-joint numbers, nothing read back
    loop         what analysis/advanced_analysis.py:430-485 does, with stochastic depth switched on so that it has something to measure:
                 30 batch-1 forwards under the context (the same multipliers, column by column), `.cpu().numpy()` after each, then np.mean
                 and np.std on the host; the two maps only

Whole calls, host clock around work that ends in a device synchronise (the loop synchronises 30 times by itself), after one untimed call
of every variant; `--rounds` timed calls per variant, the variants alternating; median and min .. max.  Before anything is timed the
ensemble's members, mean and std are compared with the loop's: a batch of 30 may take other kernel routes than a batch of 1 (tile and
fusion choices depend on the row count), so the members agree within the project's whole-model bf16 bound (max-norm 2.5e-2, tests/
test_gpu_parity.py) and the maps with them; whether they agree bit for bit is reported.  The same holds between chunk sizes, and each
chunk size is run twice to show that it repeats its own bits.

Then pk_ensemble_moments alone, by device events around `--kernel_iters` launches: the flagship stack (30 x 17 x 64 x 48) and a stack
beyond the 256 MiB Infinity Cache (L = 17 x 64 x 48 x 64 elements) in the register form (S = 30) and the two-read form (S = 40);
bandwidth = (S + 2) L 4 bytes, the traffic the algorithm needs (the two-read form's second read is not counted), over the median time.
Prints one JSON line.

    python scripts/bench_uncertainty.py [--batch_sizes 5 10 15 30] [--rounds 5] [--kernel_iters 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

H, W, K, S, SEED = 256, 192, 17, 30, 3
BF16_MAX = 2.5e-2                                                 # whole-model eval bound of tests/test_gpu_parity.py (max-norm)


def reference_loop(model, image, scales):
    """The reference's procedure, restated: one forward and one device-to-host copy per member, the statistics on the host."""
    import torch
    from infantposeestimation_gaussianbias_amd import nnops
    preds = []
    with torch.no_grad():
        for i in range(scales.shape[1]):
            with nnops.stochastic_depth(scales=scales[:, i:i + 1].contiguous()):
                preds.append(model(image)['heatmaps'].cpu().numpy())
    preds = np.array(preds)
    return preds, np.mean(preds, axis=0), np.std(preds, axis=0)


def kernel_times(torch, hipops, S_, L, iters):
    stack = torch.randn(S_, L, device="cuda")
    out = (torch.empty(L, device="cuda"), torch.empty(L, device="cuda"))
    for _ in range(3):
        hipops.ensemble_moments(stack, out=out)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        hipops.ensemble_moments(stack, out=out)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    med = float(np.median(ms))
    need = (S_ + 2) * L * 4
    return {"S": S_, "L": L, "form": "register" if S_ <= 32 else "two-read", "bytes": need, "us_median": med * 1e3, "us_min": ms[0] * 1e3,
            "us_max": ms[-1] * 1e3, "TB_per_s": need / (med * 1e-3) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_sizes", type=int, nargs="+", default=[5, 10, 15, 30])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel_iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    from infantposeestimation_gaussianbias_amd.utils import mc_uncertainty
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty: no GPU (the kernels have no CPU path)")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = PoseEstimator("hrformer_small", K, False, "fusion", True).to(dev).eval()
    image = torch.randn(1, 3, H, W, device=dev)

    def gen():
        g = torch.Generator(device=dev)
        g.manual_seed(SEED)
        return g

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, result

    variants = {f"ensemble_{b}": (lambda b=b: mc_uncertainty(model, image, S, generator=gen(), batch_size=b)) for b in args.batch_sizes}
    first = {k: timed(fn) for k, fn in variants.items()}          # untimed: code objects, weight packing, every batch shape once
    base = first[f"ensemble_{args.batch_sizes[0]}"][1]
    scales = base["scales"]
    variants["loop"] = lambda: reference_loop(model, image, scales)
    first["loop"] = timed(variants["loop"])
    preds, want_mean, want_std = first["loop"][1]
    top = float(np.abs(preds).max())
    bound = BF16_MAX * top
    same, repeats, apart = {}, {}, {}
    for k, (_, res) in first.items():
        if k == "loop":
            continue
        again = variants[k]()
        repeats[k] = all(torch.equal(again[n], res[n]) for n in res)                 # a chunk size repeats its own bits
        same[k] = all(torch.equal(res[n], base[n]) for n in ("stack", "mean", "std"))    # ... and may or may not give another's
        apart[k] = float((res["stack"] - base["stack"]).abs().max())
        assert torch.equal(res["scales"], scales) and repeats[k] and apart[k] <= bound, (k, repeats[k], apart[k], bound)
    stack = base["stack"].cpu().numpy()
    diff = {"members": float(np.abs(stack - preds[:, 0]).max()), "mean": float(np.abs(base["mean"].cpu().numpy() - want_mean[0]).max()),
            "std": float(np.abs(base["std"].cpu().numpy() - want_std[0]).max())}
    assert all(v <= bound for v in diff.values()), (diff, bound)
    assert float(base["std"].max()) > 0
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn)[0])
    out = {"model": "hrformer_small", "input": [H, W], "members": S, "rate": float(model.backbone.drop_path_rate), "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "max_abs_diff_vs_loop": diff, "diff_bound": bound, "members_abs_max": top,
           "members_bitwise_equal_to_loop": bool(np.array_equal(stack, preds[:, 0])),
           "chunks_bitwise_equal_to_first": same, "chunks_repeat_bitwise": repeats, "chunks_max_abs_diff_vs_first": apart, "first_call_ms": {k: v[0] for k, v in first.items()}}
    for k, v in t.items():
        out[f"{k}_ms_median"], out[f"{k}_ms_min"], out[f"{k}_ms_max"] = float(np.median(v)), float(min(v)), float(max(v))
    flag, big = K * (H // 4) * (W // 4), K * (H // 4) * (W // 4) * 64
    out["moments_kernel"] = [kernel_times(torch, hipops, s_, n, args.kernel_iters) for s_, n in ((30, flag), (40, flag), (30, big), (40, big))]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
