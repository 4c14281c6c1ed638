#!/usr/bin/env python3
"""Time the two entries of the localisation error analysis (pk_kpt_error, pk_kpt_error_quantiles: csrc/pk_error.hip) at K = 17 joints with
6 352 stored columns (the keypoint instances of COCO val2017) and with 100 000:

    error        pk_kpt_error on one batch of that many samples: store, 10 confidence bins, 100 confidence thresholds
    quantiles    pk_kpt_error_quantiles over the store that launch filled, 5 quantiles (grid 17 x 5)

Kernels only (the C entries called directly into preallocated outputs), device-resident inputs, device events around `--iters` back-to-back
calls after `--warmup` untimed ones, `--rounds` windows per variant with the variants alternating; median and min .. max of the per-call time.
The inputs (0.6 to 11 MB) stay in the caches between calls: warm numbers.  Before anything is timed both entries are checked against
their numpy restatement (tests/error_analysis_np.py) bit for bit.  Prints one JSON line.

    python scripts/bench_error_analysis.py [--iters 100] [--warmup 10] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from bench_grad_guard import time_steps  # noqa: E402

K, SIZES, QUANTILES = 17, (6352, 100000), (0.05, 0.25, 0.5, 0.75, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import error_analysis_np as enp
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    if not torch.cuda.is_available():
        raise SystemExit("bench_error_analysis: no GPU (the kernels have no CPU path)")
    dev = torch.device("cuda")
    up = lambda a, dt=torch.float32: torch.from_numpy(np.array(a)).to(dev, dt)      # a copy: the cached cases are read-only
    st = _lib.stream_ptr()

    def entry(name, *a):
        fn, conv = getattr(_lib.lib, name), [x.data_ptr() if hasattr(x, "data_ptr") else x for x in a] + [st]

        def call():
            if fn(*conv) != 0:
                raise RuntimeError(f"{name} failed: {_lib.lib.pk_last_error_string().decode()}")
        call.keep = a
        return call

    q = np.array(QUANTILES, np.float64)
    variants = {}
    for N in SIZES:
        pred, gt, vis, _, conf, edges, thr = enp.error_case(N, K, False, True)
        d = [up(a) for a in (pred, gt, vis, conf, edges, thr)]
        store = torch.empty(K, N, device=dev)
        buf = hipops.kpt_error_buffers(K, len(edges) - 1, len(thr), dev)
        hipops.kpt_error_accumulate(d[0], d[1], d[2], store, 0, 10.0, d[3], None, d[4], d[5], *buf)
        order, summary = hipops.kpt_error_quantiles(store, N, up(q, torch.float64))
        err = enp.errors(pred, gt, vis)
        got = store.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(err.T)) and np.array_equal(got[~np.isnan(got)], err.T[~np.isnan(err.T)]), N
        want = enp.calibration(err, conf, 10.0, edges) + (enp.pr_hist(err, conf, 10.0, thr),)
        assert all(np.array_equal(b.cpu().numpy(), w) for b, w in zip(buf, want)), N
        assert all(np.array_equal(order[k].cpu().numpy(), enp.order_stats(err[:, k], q)) for k in range(K)), N
        assert all(np.array_equal(summary[k].cpu().numpy(), enp.summary(err[:, k])) for k in range(K)), N
        dq = up(q, torch.float64)
        variants[f"error_{N}"] = entry("pk_kpt_error", d[0], d[1], d[2], d[3], None, 10.0, d[4], len(edges) - 1, d[5], len(thr), store, N,
                                       *buf, N, K)
        variants[f"quantiles_{N}"] = entry("pk_kpt_error_quantiles", store, N, N, K, dq, len(q), torch.empty_like(order),
                                           torch.empty_like(summary))
    t = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            t[k].append(time_steps(fn, args.warmup, args.iters))
    out = {"K": K, "quantiles": len(q), "iters": args.iters, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for k, v in t.items():
        out[f"{k}_us_median"], out[f"{k}_us_min"], out[f"{k}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
