#!/usr/bin/env python3
"""Time of the multi-scale merge alone (run on the GPU box, under a time limit of its own).

    timeout -k 10 300 python scripts/probes/multiscale_merge.py [--repeats 20] [--iters 400]

Workload: B = 64, K = 17, 64 x 48 maps (hrformer_base at 256 x 192), device-resident random stacks.
  ms_s3_f2    pk_multiscale_merge, scales (0.8, 1.0, 1.2), flip: reads 6 maps per output map
  ms_s1_f2    pk_multiscale_merge, scales (1.0,), flip: the arithmetic of the flip merge through the general kernel
  flip_merge  pk_flip_merge at the same size: the yardstick
HIP events around `iters` back-to-back calls, `repeats` windows per variant with the variants ALTERNATING inside every repeat; median and
min .. max of the per-call time.  Consecutive calls rotate over enough buffer sets to exceed 600 MB per variant, so that a call does not
find its inputs in the 256 MiB Infinity Cache from the call before (in use a whole forward runs between two merges).
Bytes the algorithm needs per call: (S*F + 1) * B*K*H*W * 4 (every source map read once, the output written once); the rate printed is
that figure over the measured time -- the passes that do not see a pixel are still counted, so it is a lower bound of the traffic rate.
Before anything is timed ms_s1_f2 must equal flip_merge bit for bit.  Prints readable lines and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from infantposeestimation_gaussianbias_amd import _lib  # noqa: E402
from infantposeestimation_gaussianbias_amd._lib import stream_ptr  # noqa: E402

B, K, H, W = 64, 17, 64, 48


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=400)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multiscale_merge probe: no GPU; this measurement has no CPU form")
    dev, st = torch.device("cuda"), stream_ptr()
    partner = torch.arange(K, dtype=torch.int32)
    for a in range(1, 17, 2):
        partner[a], partner[a + 1] = a + 1, a
    partner = partner.to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    map_bytes = B * K * H * W * 4

    def variant(S, scales):
        """-> (run(), algorithmic bytes per call, buffer sets)"""
        passes = S * 2
        nsets = -(-600_000_000 // ((passes + 1) * map_bytes))
        sets = [(torch.randn(passes * B, K, H, W, device=dev, generator=gen), torch.empty(B, K, H, W, device=dev)) for _ in range(nsets)]
        turn = [0]
        if scales is None:
            def run():
                turn[0] = (turn[0] + 1) % nsets
                s, o = sets[turn[0]]
                if _lib.lib.pk_flip_merge(s.data_ptr(), s[B:].data_ptr(), partner.data_ptr(), o.data_ptr(), B, K, H, W, st) != 0:
                    raise RuntimeError(_lib.lib.pk_last_error_string().decode())
        else:
            inv = (1.0 / np.asarray(scales, np.float64)).astype(np.float32)

            def run():
                turn[0] = (turn[0] + 1) % nsets
                s, o = sets[turn[0]]
                if _lib.lib.pk_multiscale_merge(s.data_ptr(), partner.data_ptr(), inv.ctypes.data, o.data_ptr(), S, 2, B, K, H, W, st) != 0:
                    raise RuntimeError(_lib.lib.pk_last_error_string().decode())
        return run, (passes + 1) * map_bytes, sets

    variants = {"ms_s3_f2": variant(3, (0.8, 1.0, 1.2)), "ms_s1_f2": variant(1, (1.0,)), "flip_merge": variant(1, None)}
    # the outputs that must agree, before anything is timed: same inputs through both kernels
    a, b = variants["ms_s1_f2"][2], variants["flip_merge"][2]
    for (sa, _), (sb, _) in zip(a, b):
        sb.copy_(sa)
    for name in ("ms_s1_f2", "flip_merge"):
        for _ in range(len(a)):
            variants[name][0]()
    torch.cuda.synchronize()
    assert all(torch.equal(oa, ob) for (_, oa), (_, ob) in zip(a, b)), "pk_multiscale_merge (S = 1, F = 2) differs from pk_flip_merge"
    for run, _, _ in variants.values():                # warm-up: code objects, clocks
        window(run, 50)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, (run, _, _) in variants.items():
            times[k].append(window(run, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "workload": f"B={B} K={K} {H}x{W}", "repeats": args.repeats, "iters": args.iters, "us": {}}
    for k, v in times.items():
        med, nbytes = statistics.median(v), variants[k][1]
        res["us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "algorithmic_bytes": nbytes,
                        "GBps": round(nbytes / med / 1e3, 1), "buffer_sets": len(variants[k][2])}
        print(f"{k:11s} {med:8.2f} us per call (min {min(v):.2f}, max {max(v):.2f})  {nbytes / 1e6:6.1f} MB needed -> {nbytes / med / 1e3:7.1f} GB/s", flush=True)
    res["ms_s1_over_flip_merge"] = round(res["us"]["ms_s1_f2"]["median"] / res["us"]["flip_merge"]["median"], 3)
    print(f"ms_s1_f2 / flip_merge {res['ms_s1_over_flip_merge']:.3f}", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
