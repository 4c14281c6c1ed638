#!/usr/bin/env python3
"""Time the per-tensor statistics (pk_tensor_stats, csrc/pk_tensor_stats.hip) on HRFormer-small's gradient buffer with the model's own
segment table and flags, by the method of scripts/bench_grad_guard.py: the variants

    tensor_stats   pk_tensor_stats: partial + finalize kernel (one record per tensor)
    with_latch     ... plus pk_tensor_stats_latch: what --trace_nonfinite adds to a step
    grad_sumsq     pk_grad_sumsq on the same buffer: it reads the same bytes (4 B/element + 1 B flag) into ONE sum
    torch_loop     torch's per-tensor loop, what a user would otherwise write: vector_norm, amax of |g| and mean per parameter view
                   (three launches or more per tensor, nothing read back)

run alternating, `--rounds` times; each timing is device events around `--iters` back-to-back calls after `--warmup` untimed ones
(the torch loop: a tenth of the iterations).  ratio_stats_over_sumsq is what the segmentation and the extra accumulators cost over a plain
read of the buffer.  Prints one JSON line.

    python scripts/bench_tensor_stats.py [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]

`--step` times the captured training step instead (HRFormer-small + fusion head, 256x192, B = 64, whole step in one hipGraph with branch
streams, as train.py --graph): three trainers from one seed -- plain, --skip_nonfinite, --skip_nonfinite --trace_nonfinite -- on the same
batch, alternating, `--rounds` times `--iters` steps each (host clock around the steps, ending in a device synchronise).
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


def time_captured_steps(args):
    import time
    import torch
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    from infantposeestimation_gaussianbias_amd.models import build_model
    cfg = get_config("hrformer_small")
    cfg.train.batch_size = 64
    batch = synthetic_batch(64, cfg.data.input_size, cfg.data.heatmap_size, 17, cfg.data.sigma, torch.device("cuda"), seed=1234)
    options = {"plain": {}, "skip_nonfinite": {"skip_nonfinite": True}, "skip_and_trace": {"skip_nonfinite": True, "trace_nonfinite": True}}
    trainers = {}
    for k, kw in options.items():
        torch.manual_seed(0)
        trainers[k] = engine.Trainer(build_model(cfg).cuda(), cfg, iters_per_epoch=1000, use_graph=True, graph_warmup=2, graph_streams=True, **kw)
        for _ in range(max(4, args.warmup)):
            trainers[k].step(batch)
        if trainers[k]._graph is None or not trainers[k]._graph_has_opt:
            raise SystemExit(f"bench_tensor_stats: {k}: the optimiser is not inside the captured step")
    t = {k: [] for k in options}
    for _ in range(args.rounds):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                tr.step(batch)
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3 / args.iters)
    if trainers["skip_and_trace"].opt.nonfinite_trace() is not None:
        raise SystemExit("bench_tensor_stats: the latch fired during the timed steps")
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"mode": "captured step, B=64, 256x192", "iters": args.iters, "rounds": args.rounds}
    for k in options:
        out[f"{k}_ms_median"], out[f"{k}_ms_all"] = med[k], [round(v, 3) for v in t[k]]
    out.update({"trace_cost_us": 1e3 * (med["skip_and_trace"] - med["skip_nonfinite"]), "device": torch.cuda.get_device_name(0)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="time the captured training step with and without the trace instead")
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
        raise SystemExit("bench_tensor_stats: no GPU (the kernels have no CPU path)")
    if args.step:
        out = time_captured_steps(args)
        line = json.dumps(out)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    torch.manual_seed(0)
    opt = engine.FlatAdamW(build_model(get_config("hrformer_small")).cuda(), skip_nonfinite=True, trace_nonfinite=True)
    n = opt.numel
    opt.grad.normal_(0.0, 1e-3)
    plan = opt._stats_plan
    views = [opt.grad_view(i) for i in range(len(opt.params))]

    def tensor_stats():
        hipops.tensor_stats(plan, opt.grad, flags=opt.flags, records=opt.trace_records)

    def with_latch():
        tensor_stats()
        hipops.tensor_stats_latch(opt.trace_records, plan.n_tensors, opt.trace_latched, opt.trace_state)

    def grad_sumsq():
        hipops.grad_sumsq(opt.grad, opt.flags, opt.guard_partials)

    def torch_loop():
        for v in views:
            torch.linalg.vector_norm(v)
            v.abs().amax()
            v.mean()

    variants = {"tensor_stats": (tensor_stats, 1), "with_latch": (with_latch, 1), "grad_sumsq": (grad_sumsq, 1), "torch_loop": (torch_loop, 10)}
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, (fn, div) in variants.items():
            t[k].append(time_steps(fn, max(1, args.warmup // div), max(1, args.iters // div)))
    if opt.nonfinite_trace() is not None:
        raise SystemExit("bench_tensor_stats: the latch fired on finite gradients")
    recs = hipops.tensor_stats_records(opt.trace_records)
    if int(recs["n"].sum()) != int((opt.flags & 2).ne(0).sum()):
        raise SystemExit("bench_tensor_stats: the records do not count the active elements")
    med = {k: float(np.median(v)) for k, v in t.items()}
    counts = np.asarray(plan.counts)
    out = {"numel": n, "n_tensors": plan.n_tensors, "n_items": plan.n_items, "chunk_elems": hipops.tensor_stats_chunk_elems(),
           "tensors_le_256": int((counts <= 256).sum()), "largest_tensor": int(counts.max()), "iters": args.iters, "rounds": args.rounds}
    for k in variants:
        out[f"{k}_us_median"], out[f"{k}_us_min"], out[f"{k}_us_max"] = med[k], float(min(t[k])), float(max(t[k]))
        out[f"{k}_us_all"] = [round(v, 2) for v in t[k]]
    out.update({"ratio_stats_over_sumsq": med["tensor_stats"] / med["grad_sumsq"], "ratio_torch_loop_over_stats": med["torch_loop"] / med["tensor_stats"],
                "tensor_stats_GBps": 5.0 * n / med["tensor_stats"] * 1e-3, "grad_sumsq_GBps": 5.0 * n / med["grad_sumsq"] * 1e-3,
                "device": torch.cuda.get_device_name(0)})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
