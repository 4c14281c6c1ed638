#!/usr/bin/env python3
"""Time the two entries of the activation statistics (pk_activation_stats, pk_activation_quantiles: csrc/pk_activation.hip) on feature maps
of the sizes a batch of 64 crops of 256 x 192 produces (rows x channels, post-ReLU: about half the elements are +0), against the
reference's way on the same tensors (analysis/advanced_analysis.py: a forward hook's `output.detach().cpu()`, then the per-channel mean and
`np.sort` over the whole tensor on the host):

    stats        pk_activation_stats: per-channel records and the 4096-bin table, two launches
    quantiles    pk_activation_quantiles over that table, 3 quantiles, three launches
    host         x.float().cpu() (a synchronising copy), numpy mean over the rows, np.sort of the flattened tensor

Kernels: the op-layer calls into preallocated workspaces, device events around `--iters` back-to-back calls after `--warmup` untimed ones,
`--rounds` windows per variant with the variants alternating; median and min .. max of the per-call time, and the bytes of x over the
median as GB/s.  Tensors up to 256 MiB stay in the last-level cache between calls: warm numbers, to be read next to the chip's 8.0 TB/s
HBM peak (6.29 TB/s measured for a copy), not as a share of it.  The host way is timed with the host clock, `--host-reps` times, the
minimum kept.  Before anything is timed both entries are checked against their numpy restatement (tests/activation_np.py) bit for bit on
the smallest shape.  Prints one JSON line.

    python scripts/bench_activation_stats.py [--iters 50] [--warmup 5] [--rounds 5] [--host-reps 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from bench_grad_guard import time_steps  # noqa: E402

# (rows, channels): B = 64 at 256 x 192 -- the four branch resolutions of HRNet-W32 / HRFormer, the stem, and layer1's 256-channel map
SHAPES = ((64 * 8 * 6, 256), (64 * 16 * 12, 128), (64 * 32 * 24, 64), (64 * 64 * 48, 32), (64 * 64 * 48, 64), (64 * 64 * 48, 256))
QUANTILES = (0.25, 0.5, 0.75)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import activation_np as anp
    from infantposeestimation_gaussianbias_amd import hipops
    if not torch.cuda.is_available():
        raise SystemExit("bench_activation_stats: no GPU (the kernels have no CPU path)")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    variants, host, tensors = {}, {}, {}
    for M, C in SHAPES:
        x = torch.relu(torch.randn(M, C, device=dev, generator=g)).to(torch.bfloat16)
        tensors[(M, C)] = x
        rec, hist = hipops.activation_stats(x)
        order = hipops.activation_quantiles(x, hist, QUANTILES)
        if (M, C) == SHAPES[0]:
            bits = x.view(torch.int16).cpu().numpy().view(np.uint16)
            want_rec, want_hist = anp.stats(bits)
            got = hipops.activation_records(rec)
            assert np.array_equal(hist.cpu().numpy(), want_hist) and all(np.array_equal(got[k], want_rec[k]) for k in want_rec.dtype.names)
            assert np.array_equal(order.cpu().numpy(), anp.quantiles(bits, QUANTILES))
        variants[f"stats_{M}x{C}"] = lambda x=x: hipops.activation_stats(x)
        variants[f"quantiles_{M}x{C}"] = lambda x=x, hist=hist: hipops.activation_quantiles(x, hist, QUANTILES)

        def host_way(x=x):
            t0 = time.perf_counter()
            a = x.float().cpu().numpy()
            mean, ordered = a.mean(axis=0), np.sort(a.reshape(-1))
            return (time.perf_counter() - t0) * 1e6, mean, ordered

        best, mean, ordered = min((host_way() for _ in range(args.host_reps)), key=lambda r: r[0])
        host[(M, C)] = best
        # the same numbers: channel means to fp32 summation error, the median exactly
        r = hipops.activation_records(rec)
        assert np.allclose(r["sum"] / r["n"], mean, rtol=1e-3, atol=1e-6)
        lo, hi = order.cpu().numpy()[1]
        n = ordered.size
        assert lo == ordered[(n - 1) // 2] and hi == ordered[min((n - 1) // 2 + 1, n - 1)]
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(time_steps(fn, args.warmup, args.iters))
    out = {"quantiles": len(QUANTILES), "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": []}
    for M, C in SHAPES:
        nbytes = 2 * M * C
        row = {"rows": M, "channels": C, "mbytes": nbytes / 1e6, "host_us": host[(M, C)]}
        for kind in ("stats", "quantiles"):
            v = t[f"{kind}_{M}x{C}"]
            row[f"{kind}_us_median"], row[f"{kind}_us_min"], row[f"{kind}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
            row[f"{kind}_gbps"] = nbytes / (np.median(v) * 1e-6) / 1e9
        row["host_over_device"] = host[(M, C)] / (row["stats_us_median"] + row["quantiles_us_median"])
        out["shapes"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
