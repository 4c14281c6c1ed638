#!/usr/bin/env python3
"""Cost of the per-person heatmap overlay (run on the GPU box, under a time limit of its own).

    timeout -k 10 300 python scripts/bench_overlay_patches.py [--repeats 20] [--iters 200]

Workload: 64 frames of 640 x 480, 4 persons each (256 patches), heatmaps 64 x 48 x 17; the crops are person-sized boxes spread over the
frame (scale 150..330 px wide, 3:4), a quarter of them rotated.
  * kernels only, device-resident inputs, HIP events around `iters` back-to-back calls, `repeats` windows per variant with the variants
    ALTERNATING inside every repeat; median and min .. max of the per-call time:
      patches   pk_heatmap_overlay_patches   (max over K, per-patch min / max, tile gather + blend: three launches)
      whole     pk_heatmap_overlay           (the existing whole-frame overlay on the same frames, one stack per frame: the yardstick)
    Both blend in place, so the frames change from call to call; the time does not depend on their bytes.  Consecutive calls ROTATE over 4
    sets of frames (59 MB per set), so a call does not find its frames in the Infinity Cache from the call before.
  * the whole `draw_person_heatmaps` call on a device batch (copy of the batch, matrices on the host, the small uploads, launches; host
    clock around a device synchronise).
Before anything is timed the two runs of the patch overlay on the same inputs must agree bit for bit.
Prints readable lines and one JSON line.  Bytes the patch path needs per call: P K h w 4 read once (13.4 MB), P h w 4 written and read
back (3.1 MB), and 6 bytes per covered pixel of the frames.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infantposeestimation_gaussianbias_amd import _lib  # noqa: E402
from infantposeestimation_gaussianbias_amd._lib import stream_ptr  # noqa: E402
from infantposeestimation_gaussianbias_amd.utils import visualization as V  # noqa: E402

N, H, W, PER, K, h, w = 64, 480, 640, 4, 17, 64, 48


def inputs(seed=0):
    rng = np.random.default_rng(seed)
    P = N * PER
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    hm = rng.random((P, K, h, w), dtype=np.float32)
    centers = np.stack([rng.uniform(80, W - 80, P), rng.uniform(100, H - 100, P)], 1)
    sx = rng.uniform(150, 330, P)
    scales = np.stack([sx, sx * 4 / 3], 1)
    rot = np.where(rng.random(P) < 0.25, rng.uniform(-40, 40, P), 0.0)
    return frames, hm, np.repeat(np.arange(N, dtype=np.int32), PER), V.crop_heatmap_matrices(centers, scales, (w, h), rot), centers, scales, rot


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
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_overlay_patches: no GPU; this measurement has no CPU form")
    dev = torch.device("cuda")
    frames, hm, idx, mats, centers, scales, rot = inputs()
    P = len(idx)
    L = _lib.lib
    SETS = 4
    f0 = torch.from_numpy(frames).to(dev)
    sets = [f0.clone() for _ in range(SETS)]
    hm_p = torch.from_numpy(hm).to(dev)
    hm_n = hm_p[::PER].contiguous()                         # one stack per frame for the whole-frame overlay
    idx_d, mat_d = torch.from_numpy(idx).to(dev), torch.from_numpy(np.ascontiguousarray(mats.reshape(P, 6))).to(dev)
    lut = torch.from_numpy(V.heatmap_lut()).to(dev)
    ws_p = torch.empty(L.pk_heatmap_overlay_patches_ws_floats(P, K, h, w), dtype=torch.float32, device=dev)
    ws_n = torch.empty(L.pk_heatmap_overlay_ws_floats(N, K, h, w, H, W), dtype=torch.float32, device=dev)
    cover = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    st = stream_ptr()
    turn = [0]

    def patches(cov=None):
        turn[0] = (turn[0] + 1) % SETS
        if L.pk_heatmap_overlay_patches(sets[turn[0]].data_ptr(), hm_p.data_ptr(), idx_d.data_ptr(), mat_d.data_ptr(), 0.5, lut.data_ptr(), None,
                                        cov, ws_p.data_ptr(), N, P, K, h, w, H, W, st) != 0:
            raise RuntimeError(f"pk_heatmap_overlay_patches failed: {L.pk_last_error_string().decode()}")

    def whole():
        turn[0] = (turn[0] + 1) % SETS
        if L.pk_heatmap_overlay(sets[turn[0]].data_ptr(), hm_n.data_ptr(), 0.5, lut.data_ptr(), None, ws_n.data_ptr(), N, K, h, w, H, W, st) != 0:
            raise RuntimeError(f"pk_heatmap_overlay failed: {L.pk_last_error_string().decode()}")

    # two runs on the same inputs agree bit for bit; how much of the frames the patches cover
    turn[0] = 0
    patches(cover.data_ptr())
    turn[0] = 1
    patches()
    torch.cuda.synchronize()
    assert torch.equal(sets[1], sets[2]) and not torch.equal(sets[1], f0), "two runs of the patch overlay differ"
    covered = float((cover > 0).float().mean())
    variants = {"patches": patches, "whole": whole}
    for fn in variants.values():                     # warm-up: code objects, clocks
        window(fn, 50)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "workload": f"{N} x {W}x{H}, {PER} persons each, heatmaps {h}x{w}x{K}",
           "covered_share": round(covered, 4), "repeats": args.repeats, "iters": args.iters, "buffer_sets": SETS, "kernel_us": {}}
    for k, v in times.items():
        med = statistics.median(v)
        res["kernel_us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        print(f"{k:8s} {med:8.2f} us per call (min {min(v):.2f}, max {max(v):.2f})", flush=True)
    res["patches_over_whole"] = round(res["kernel_us"]["patches"]["median"] / res["kernel_us"]["whole"]["median"], 3)
    print(f"covered share of the frames {covered:.3f}   patches / whole {res['patches_over_whole']:.3f}", flush=True)

    # the whole visualization call on a device batch
    for _ in range(3):
        V.draw_person_heatmaps(f0, hm_p, centers=centers, scales=scales, rotations=rot, image_index=idx)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        V.draw_person_heatmaps(f0, hm_p, centers=centers, scales=scales, rotations=rot, image_index=idx)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    res["draw_person_heatmaps_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
    print(f"draw_person_heatmaps {statistics.median(ts):.3f} ms per {N} frames (min {min(ts):.3f}, max {max(ts):.3f})", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
