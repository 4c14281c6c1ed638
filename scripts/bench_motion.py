#!/usr/bin/env python3
"""Cost of the movement-analysis and PCK kernels (run on the GPU box, under a time limit of its own).

    timeout -k 10 300 python scripts/bench_motion.py [--repeats 10] [--iters 100]

Workloads:
  * pk_motion_stats and pk_position_histogram (640 x 480 frame, 10-px bins: 64 x 48) on (S, T, K) = (1, 18000, 17), ten minutes of one
    infant at 30 frames a second, and (64, 900, 13), 64 clips of half a minute; with confidences;
  * pk_motion_spectrum (both launches) on the same two shapes, a band of 256 bins under the Hann window: bins 300 .. 555 of an 18 000-point
    transform (0.5 to 0.925 Hz at 30 frames a second) and bins 1 .. 256 of a 1024-point one (zero-padded clips);
  * pk_pck on N = 6352 instances of K = 17 joints (the person instances of COCO val2017) at 6 thresholds.
Kernels only (the C entries called directly into preallocated outputs), device-resident inputs, HIP events around `iters` back-to-back calls, `repeats` windows per variant with the variants
ALTERNATING inside every repeat; median and min .. max of the per-call time.  The inputs are small (2.5 to 8 MB) and stay in the caches
between calls: these are warm numbers, which is how a report over one trajectory calls the kernels (statistics, then histogram, on the same
tensor).  Before anything is timed every kernel is checked against its numpy restatement (tests/motion_np.py, tests/spectrum_np.py), and the restatement is timed on
the host of the same box (best of 3) for scale.  Prints readable lines and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motion_np as mnp  # noqa: E402
import spectrum_np as snp  # noqa: E402
from infantposeestimation_gaussianbias_amd import _lib, hipops  # noqa: E402
from infantposeestimation_gaussianbias_amd._lib import stream_ptr  # noqa: E402

W, H, BIN = 640, 480, 10
SHAPES = [(1, 18000, 17), (64, 900, 13)]
SPECTRUM = {(1, 18000, 17): (18000, 300, 256), (64, 900, 13): (1024, 1, 256)}      # (S, T, K) -> n_fft, first bin, bins
PCK_N, PCK_K, PCK_THR = 6352, 17, 6


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def entry(name, *args):
    """-> a call of the C entry `name` on the current stream with these arguments (tensors by pointer; they stay alive in the closure)."""
    fn, st = getattr(_lib.lib, name), stream_ptr()
    conv = [a.data_ptr() if hasattr(a, "data_ptr") else a for a in args] + [st]

    def call():
        if fn(*conv) != 0:
            raise RuntimeError(f"{name} failed: {_lib.lib.pk_last_error_string().decode()}")
    call.keep = args
    return call


def host_ms(fn):
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def trajectories(S, T, K, seed):
    g = np.random.default_rng(seed)
    c = (np.array([W / 2, H / 2]) + np.cumsum(g.standard_normal((S, T, K, 2)) * 1.5, axis=1)).astype(np.float32)
    return c, g.random((S, T, K)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_motion: no GPU; this measurement has no CPU form")
    dev = torch.device("cuda")
    ex, ey = np.linspace(0, W, W // BIN + 1), np.linspace(0, H, H // BIN + 1)
    dex, dey = torch.from_numpy(ex).to(dev), torch.from_numpy(ey).to(dev)
    variants, host, checks = {}, {}, {}
    for S, T, K in SHAPES:
        c, conf = trajectories(S, T, K, S + T)
        dc, dconf = torch.from_numpy(c).to(dev), torch.from_numpy(conf).to(dev)
        tag = f"{S}x{T}x{K}"
        want = mnp.motion_stats(c, conf, 0.3)
        got = hipops.motion_stats(dc, dconf, 0.3).cpu().numpy()
        exact = all(np.array_equal(got[..., i], want[..., i]) for i in (0, 1, 2, 3, 4, 7, 10))
        rel = max(float(np.max(np.abs(got[..., i] - want[..., i]) / np.maximum(np.abs(want[..., i]), 1e-300))) for i in (5, 6, 8, 9))
        assert exact and rel <= (T + 16) * 2.0 ** -52, (tag, exact, rel)
        assert np.array_equal(hipops.position_histogram(dc, dex, dey, dconf, 0.3).cpu().numpy(), mnp.histogram2d(c, ex, ey, conf, 0.3)), tag
        checks[tag] = {"stats_rel_err": rel}
        stats = torch.empty(S, K, 11, dtype=torch.float64, device=dev)
        counts = torch.empty(S, K, H // BIN, W // BIN, dtype=torch.int32, device=dev)
        variants[f"motion_stats {tag}"] = entry("pk_motion_stats", dc, dconf, stats, S, T, K, 0.3)
        variants[f"position_histogram {tag}"] = entry("pk_position_histogram", dc, dconf, dex, dey, counts, S, T, K, W // BIN, H // BIN, 0.3)
        host[f"motion_stats {tag}"] = host_ms(lambda: mnp.motion_stats(c, conf, 0.3))
        host[f"position_histogram {tag}"] = host_ms(lambda: mnp.histogram2d(c, ex, ey, conf, 0.3))
        n_fft, j0, nb = SPECTRUM[(S, T, K)]
        p_want, n_valid, _, scale = snp.power(c, conf, 0.3, n_fft, j0, nb, 1)
        p_got, s_got = (t.cpu().numpy() for t in hipops.motion_spectrum(dc, dconf, 0.3, n_fft, j0, nb, 1))
        share = float((np.abs(p_got - p_want) / ((n_valid + 16) * 2.0 ** -50 * scale)[..., None]).max())      # of the tests' bound
        assert share <= 1.0 and np.array_equal(s_got[..., 0], n_valid), (tag, share)
        checks[tag]["spectrum_err_share_of_bound"] = share
        power = torch.empty(S, K, nb, dtype=torch.float64, device=dev)
        summary = torch.empty(S, K, 6, dtype=torch.float64, device=dev)
        variants[f"motion_spectrum {tag} {nb} bins"] = entry("pk_motion_spectrum", dc, dconf, power, summary, S, T, K, 0.3, n_fft, j0, nb, 1)
        host[f"motion_spectrum {tag} {nb} bins"] = host_ms(lambda: snp.spectrum(c, conf, 0.3, n_fft, j0, nb, 1))
    g = np.random.default_rng(3)
    gt = (g.random((PCK_N, PCK_K, 2)) * [W, H]).astype(np.float32)
    norm = (g.random(PCK_N) * 300 + 30).astype(np.float32)
    pred = (gt + g.standard_normal(gt.shape) * norm[:, None, None] * 0.2).astype(np.float32)
    vis = g.integers(0, 3, (PCK_N, PCK_K)).astype(np.float32)
    thr = np.linspace(0.05, 0.5, PCK_THR).astype(np.float32)
    d = [torch.from_numpy(a).to(dev) for a in (pred, gt, vis, norm, thr)]
    buf = hipops.pck_buffers(PCK_K, PCK_THR, dev)
    hipops.pck_accumulate(*d, *buf)
    correct, valid, err = mnp.pck(pred, gt, vis, norm, thr)
    assert np.array_equal(buf[0].cpu().numpy(), correct) and np.array_equal(buf[1].cpu().numpy(), valid)
    tag = f"pck {PCK_N}x{PCK_K}, {PCK_THR} thresholds"
    variants[tag] = entry("pk_pck", *d, *buf, PCK_N, PCK_K, PCK_THR)
    host[tag] = host_ms(lambda: mnp.pck(pred, gt, vis, norm, thr))

    for fn in variants.values():                     # warm-up: code objects, clocks
        window(fn, 20)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "iters": args.iters, "checks": checks, "call_us": {},
           "host_numpy_ms": {k: round(v, 3) for k, v in host.items()}}
    for k, v in times.items():
        med = statistics.median(v)
        res["call_us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        print(f"{k:40s} {med:9.2f} us per call (min {min(v):.2f}, max {max(v):.2f})   numpy on the host {host[k]:9.3f} ms", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
