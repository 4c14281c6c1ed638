#!/usr/bin/env python3
"""Time the guarded optimiser step (pk_grad_sumsq + pk_grad_guard_finalize + pk_adamw_step_guarded, csrc/pk_optim.hip) against
pk_adamw_step alone on HRFormer-small's flat parameter buffer (FlatAdamW(model).numel elements, the model's own flags).  Both variants
run on the same buffers, alternating, `--rounds` times; each timing is device events around `--iters` back-to-back steps after
`--warmup` untimed ones.  The guarded step reads the gradient once more (4 B/element on top of the update's 28 B/element, the bf16 copy
is not written here, as in training) and adds two small launches, so the expectation -- not a measurement -- is (28 + 4) / 28 = 1.14
plus launch gaps.  Prints one JSON line.

    python scripts/bench_grad_guard.py [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_steps(fn, warmup, iters):
    """us per call: device events around `iters` calls on the current stream."""
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


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
        raise SystemExit("bench_grad_guard: no GPU (the kernels have no CPU path)")
    torch.manual_seed(0)
    opt = engine.FlatAdamW(build_model(get_config("hrformer_small")).cuda(), clip_grad_norm=1.0)
    n = opt.numel
    opt.grad.normal_(0.0, 1e-3)                    # finite gradients: the guarded step applies every update, as the plain one does
    opt.lr_dev.fill_(1e-6)
    b1, b2 = opt.betas

    def plain():
        hipops.adamw_step(opt.flat, opt.grad, opt.exp_avg, opt.exp_avg_sq, opt.flags, None, opt.lr_dev, opt.step_dev, b1, b2, opt.eps,
                          opt.weight_decay, 1.0)

    def guarded():
        hipops.grad_sumsq(opt.grad, opt.flags, opt.guard_partials)
        hipops.grad_guard_finalize(opt.guard_partials, 1.0, opt.clip_grad_norm, opt.guard_state, opt.step_dev)
        hipops.adamw_step_guarded(opt.flat, opt.grad, opt.exp_avg, opt.exp_avg_sq, opt.flags, None, opt.lr_dev, opt.step_dev, b1, b2,
                                  opt.eps, opt.weight_decay, opt.guard_state, 1.0)

    def sumsq_only():
        hipops.grad_sumsq(opt.grad, opt.flags, opt.guard_partials)

    opt.step_dev.fill_(1)
    t = {"plain": [], "guarded": [], "sumsq": []}
    for _ in range(args.rounds):
        t["plain"].append(time_steps(plain, args.warmup, args.iters))
        t["guarded"].append(time_steps(guarded, args.warmup, args.iters))
        t["sumsq"].append(time_steps(sumsq_only, args.warmup, args.iters))
    stats = opt.guard_stats()
    if stats["skipped_steps"] or not np.isfinite(stats["grad_norm"]):
        raise SystemExit(f"bench_grad_guard: the timed guarded steps were not all applied: {stats}")
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"numel": n, "iters": args.iters, "rounds": args.rounds,
           "adamw_step_us_median": med["plain"], "adamw_step_us_all": [round(v, 2) for v in t["plain"]],
           "guarded_step_us_median": med["guarded"], "guarded_step_us_all": [round(v, 2) for v in t["guarded"]],
           "grad_sumsq_us_median": med["sumsq"], "ratio_guarded_over_plain": med["guarded"] / med["plain"],
           "expected_ratio_bytes_only": 32.0 / 28.0,
           "adamw_step_GBps": 28.0 * n / med["plain"] * 1e-3, "grad_sumsq_GBps": 5.0 * n / med["sumsq"] * 1e-3,
           "grad_norm": stats["grad_norm"], "clip_coef": stats["clip_coef"], "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
