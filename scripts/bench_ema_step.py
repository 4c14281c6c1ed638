#!/usr/bin/env python3
"""Time the optimiser step with and without the weight EMA (pk_adamw_step_ema, csrc/pk_optim.hip) on HRFormer-small's flat parameter
buffer (FlatAdamW(model).numel elements, the model's own flags), by the method of scripts/bench_grad_guard.py: the four variants

    plain          pk_adamw_step
    ema            pk_adamw_step_ema, guard_state NULL
    guarded        pk_grad_sumsq + pk_grad_guard_finalize + pk_adamw_step_guarded
    guarded_ema    pk_grad_sumsq + pk_grad_guard_finalize + pk_adamw_step_ema

run on the same buffers, alternating, `--rounds` times; each timing is device events around `--iters` back-to-back steps after `--warmup`
untimed ones.  The EMA reads and writes one more fp32 buffer (8 B/element on top of the update's 28 B/element; the bf16 copy is not
written here, as in training), so the expectation -- not a measurement -- is 36 / 28 = 1.29 for the unguarded pair.  Prints one JSON line.

    python scripts/bench_ema_step.py [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd import engine, hipops
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.models import build_model
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema_step: no GPU (the kernels have no CPU path)")
    torch.manual_seed(0)
    opt = engine.FlatAdamW(build_model(get_config("hrformer_small")).cuda(), clip_grad_norm=1.0, ema_decay=0.9998)
    n = opt.numel
    opt.grad.normal_(0.0, 1e-3)                    # finite gradients: the guarded steps apply every update, as the plain ones do
    opt.lr_dev.fill_(1e-6)
    b1, b2 = opt.betas
    common = (opt.flat, opt.grad, opt.exp_avg, opt.exp_avg_sq, opt.flags, None, opt.lr_dev, opt.step_dev, b1, b2, opt.eps, opt.weight_decay)

    def guard():
        hipops.grad_sumsq(opt.grad, opt.flags, opt.guard_partials)
        hipops.grad_guard_finalize(opt.guard_partials, 1.0, opt.clip_grad_norm, opt.guard_state, opt.step_dev)

    def plain():
        hipops.adamw_step(*common, 1.0)

    def ema():
        hipops.adamw_step_ema(*common, None, opt.ema, opt.ema_decay, 1.0)

    def guarded():
        guard()
        hipops.adamw_step_guarded(*common, opt.guard_state, 1.0)

    def guarded_ema():
        guard()
        hipops.adamw_step_ema(*common, opt.guard_state, opt.ema, opt.ema_decay, 1.0)

    variants = {"plain": plain, "ema": ema, "guarded": guarded, "guarded_ema": guarded_ema}
    opt.step_dev.fill_(1)
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(time_steps(fn, args.warmup, args.iters))
    stats = opt.guard_stats()
    if stats["skipped_steps"] or not np.isfinite(stats["grad_norm"]) or not bool(torch.isfinite(opt.ema).all()):
        raise SystemExit(f"bench_ema_step: the timed guarded steps were not all applied, or the average is not finite: {stats}")
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"numel": n, "iters": args.iters, "rounds": args.rounds}
    for k in variants:
        out[f"{k}_us_median"], out[f"{k}_us_min"], out[f"{k}_us_max"] = med[k], float(min(t[k])), float(max(t[k]))
        out[f"{k}_us_all"] = [round(v, 2) for v in t[k]]
    out.update({"ratio_ema_over_plain": med["ema"] / med["plain"], "ratio_guarded_ema_over_guarded": med["guarded_ema"] / med["guarded"],
                "expected_ratio_bytes_only": 36.0 / 28.0, "plain_GBps": 28.0 * n / med["plain"] * 1e-3,
                "ema_GBps": 36.0 * n / med["ema"] * 1e-3, "device": torch.cuda.get_device_name(0)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
