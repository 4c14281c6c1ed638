#!/usr/bin/env python3
"""Cost of the colour jitter in the device input pipeline (run on the GPU box, under a time limit of its own).

    timeout -k 10 300 python scripts/bench_color_jitter.py [--baseline-lib OTHER/libposekernels.so] [--repeats 20] [--iters 400]

Workload: 64 images of 640 x 480 cropped to 256 x 192, both outputs (fp32 NCHW + bf16 NHWC-8) on.
  * kernels only, device-resident inputs, HIP events around `iters` back-to-back calls, `repeats` windows per variant with the variants
    ALTERNATING inside every repeat; median and min .. max of the per-call time:
      plain     pk_affine_crop_normalize                       (one launch)
      jitter    pk_affine_crop_jitter_normalize, all enabled   (two launches)
      baseline  pk_affine_crop_normalize of --baseline-lib     (another build of the library, e.g. the parent commit's; loaded with
                                                                ctypes only, so it need not export the jitter entry)
    Consecutive calls ROTATE over 4 sets of source / output / workspace buffers (160 MB per set): a call's 60 MB of source, 88 MB of
    output and 12.6 MB of scratch would otherwise sit in the 256 MiB Infinity Cache from one call to the next, which a training step
    between two crops does not allow.  (The scratch written by the first launch of a call is still read back by its second launch
    while it may be cache-resident, as in real use.)
  * the whole DeviceCropper call (staging, the one host-to-device copy, launches; host clock around a device synchronise), plain and
    with every sample jittered: the figure DESIGN.md quotes next to the training step's img/s.
Before anything is timed, the jitter entry with every sample disabled and the baseline build must reproduce the plain crop bit for bit.
Prints readable lines and one JSON line.  Bytes per output pixel the algorithm needs: 28 written (12 + 16) by the plain path; the
jitter path adds 4 written + 4 read of scratch.
"""
import argparse
import ctypes
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
from infantposeestimation_gaussianbias_amd.datasets import transforms as T  # noqa: E402

B, SRC_W, SRC_H, W, H = 64, 640, 480, 192, 256


def inputs(seed=0):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(B)]
    mats, flips = [], []
    for _ in range(B):
        c = np.array([SRC_W / 2 + rng.uniform(-60, 60), SRC_H / 2 + rng.uniform(-40, 40)], np.float32)
        s = np.array([300.0, 400.0], np.float32) * rng.uniform(0.7, 1.3)
        mats.append(T.get_affine_matrix(c, s, (W, H), rng.uniform(-40, 40)))
        flips.append(bool(rng.integers(0, 2)))
    jit = [tuple(1 + rng.uniform(-r, r) for r in (0.3, 0.3, 0.2)) for _ in range(B)]
    return imgs, mats, flips, jit


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
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=400)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_color_jitter: no GPU; this measurement has no CPU form")
    dev = torch.device("cuda")
    imgs, mats, flips, jit = inputs()
    desc = np.zeros(B, T._CROP_DTYPE)
    for i, im in enumerate(imgs):
        desc[i] = (i * im.size, SRC_H, SRC_W, int(flips[i]), 0, T.invert_affine(mats[i]))
    SETS = 4
    src0 = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    dtab = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    jt = np.zeros(B, T._JITTER_DTYPE)
    for i, j in enumerate(jit):
        jt[i] = (1, *j)
    jon = torch.from_numpy(jt.view(np.uint8).copy()).to(dev)
    joff = torch.zeros_like(jon)
    ws_bytes = _lib.lib.pk_affine_crop_jitter_ws_bytes(B, W, H)
    sets = [(src0.clone(), torch.empty(B, 3, H, W, dtype=torch.float32, device=dev), torch.empty(B, H, W, 8, dtype=torch.bfloat16, device=dev),
             torch.empty(ws_bytes, dtype=torch.uint8, device=dev)) for _ in range(SETS)]
    mean, std, st = T.MEAN.ctypes.data, T.STD.ctypes.data, stream_ptr()

    def rotating(fn, arg_sets, what):
        turn = [0]

        def run():
            turn[0] = (turn[0] + 1) % SETS
            if fn(*arg_sets[turn[0]]) != 0:
                raise RuntimeError(f"{what} failed: {_lib.lib.pk_last_error_string().decode()}")
        return run

    def plain_of(lib):
        return rotating(lib.pk_affine_crop_normalize,
                        [(s.data_ptr(), dtab.data_ptr(), B, W, H, o32.data_ptr(), o16.data_ptr(), mean, std, st) for s, o32, o16, _ in sets],
                        "pk_affine_crop_normalize")

    def jitter_of(table):
        return rotating(_lib.lib.pk_affine_crop_jitter_normalize,
                        [(s.data_ptr(), dtab.data_ptr(), table.data_ptr(), B, W, H, o32.data_ptr(), o16.data_ptr(), mean, std, ws.data_ptr(), ws.numel(), st)
                         for s, o32, o16, ws in sets], "pk_affine_crop_jitter_normalize")

    variants = {"plain": plain_of(_lib.lib), "jitter": jitter_of(jon)}
    guards = {"jitter entry with every sample disabled": jitter_of(joff)}
    if args.baseline_lib:
        other = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        other.pk_affine_crop_normalize.argtypes = _lib.declared_symbols()["pk_affine_crop_normalize"][1]
        other.pk_affine_crop_normalize.restype = ctypes.c_int
        variants["baseline"] = guards["baseline build"] = plain_of(other)
    # the outputs that must agree, before anything is timed
    for _ in range(SETS):
        variants["plain"]()
    ref = [(o32.clone(), o16.clone()) for _, o32, o16, _ in sets]
    for name, fn in guards.items():
        for _, o32, o16, _ in sets:
            o32.zero_(), o16.zero_()
        for _ in range(SETS):
            fn()
        for (r32, r16), (_, o32, o16, _) in zip(ref, sets):
            assert torch.equal(o32, r32) and torch.equal(o16, r16), f"{name} does not reproduce the plain crop"
    variants["jitter"]()
    assert not torch.equal(sets[1][1], ref[1][0]), "the jitter path left the crop unchanged"
    for fn in variants.values():                     # warm-up: code objects, clocks
        window(fn, 50)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "workload": f"{B} x {SRC_W}x{SRC_H} -> {W}x{H}, fp32 NCHW + bf16 NHWC-8",
           "repeats": args.repeats, "iters": args.iters, "buffer_sets": SETS, "kernel_us": {}}
    px = B * W * H
    for k, v in times.items():
        med = statistics.median(v)
        res["kernel_us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        nbytes = px * (28 + (8 if k == "jitter" else 0))
        print(f"{k:9s} {med:8.2f} us per call (min {min(v):.2f}, max {max(v):.2f})  {nbytes / med / 1e3:7.1f} GB/s of output + scratch traffic", flush=True)
    res["jitter_over_plain"] = round(res["kernel_us"]["jitter"]["median"] / res["kernel_us"]["plain"]["median"], 3)
    line = f"jitter / plain {res['jitter_over_plain']:.3f}"
    if "baseline" in res["kernel_us"]:
        res["jitter_over_baseline"] = round(res["kernel_us"]["jitter"]["median"] / res["kernel_us"]["baseline"]["median"], 3)
        line += f"   jitter / baseline {res['jitter_over_baseline']:.3f}"
    print(line, flush=True)

    # the whole DeviceCropper call: staging + one copy + launches
    crop = T.DeviceCropper((W, H), dev)
    res["cropper_ms"] = {}
    for name, j in (("plain", None), ("jitter", jit)):
        for _ in range(5):
            crop(imgs, mats, flips, jitter=j)
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            crop(imgs, mats, flips, jitter=j)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        res["cropper_ms"][name] = {"median": round(med, 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "img_per_s": round(B / med * 1e3)}
        print(f"DeviceCropper {name:6s} {med:.3f} ms per {B} images (min {min(ts):.3f}, max {max(ts):.3f}) = {B / med * 1e3:.0f} img/s", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
