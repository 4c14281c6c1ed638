#!/usr/bin/env python3
"""Cost of the occlusion / blur / noise augmentation in the device input pipeline (run on the GPU box, under a time limit of its own).

    timeout -k 10 300 python scripts/bench_augment.py [--baseline-lib OTHER/libposekernels.so] [--repeats 20] [--iters 400]

Workload and method of scripts/bench_color_jitter.py: 64 images of 640 x 480 cropped to 256 x 192, both outputs (fp32 NCHW + bf16
NHWC-8) on.
  * kernels only, device-resident inputs, HIP events around `iters` back-to-back calls, `repeats` windows per variant with the variants
    ALTERNATING inside every repeat; median and min .. max of the per-call time; consecutive calls ROTATE over 4 sets of source / output /
    workspace buffers (160 MB per set), so that no call finds its predecessor's data in the 256 MiB Infinity Cache:
      plain     pk_affine_crop_normalize                                        (one launch)
      jitter    pk_affine_crop_jitter_normalize, all enabled                    (two launches)
      augment   pk_affine_crop_augment_normalize, every stage on every sample   (two launches): jitter, blur sigma 2.5 (R = 7), noise,
                four rectangles of both fill modes
      blur_off  the same entry with only jitter and noise on                    (what the LDS passes cost is augment - blur_off)
      baseline  pk_affine_crop_normalize of --baseline-lib   (another build of the library, e.g. the parent commit's; ctypes only)
  * the whole DeviceCropper call (staging, the one host-to-device copy, launches; host clock around a device synchronise): plain, jittered
    and fully augmented, the figure DESIGN.md quotes next to the training step's img/s.
Before anything is timed, the new entry with every stage off and the baseline build must reproduce the plain crop bit for bit, and the
new entry with only the jitter on must reproduce the jitter entry.  Prints readable lines and one JSON line.
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
    rs = np.random.RandomState(seed)
    occ = T.RandomOcclusion(prob=1.0, max_rects=4, rng=rs, input_size=(W, H))
    full = []
    for i in range(B):
        o = occ({})["occlusion"]
        while len(o["rects"]) < 4:                     # always four rectangles, both fill modes
            o["rects"].append(o["rects"][-1])
        o["mode"], o["rgb"] = [1, 0, 1, 0], [(0, 0, 0), T.MEAN_FILL, (0, 0, 0), T.MEAN_FILL]
        full.append({"blur": 2.5, "noise": (8.0, 1000 + i), "occlusion": o})
    return imgs, mats, flips, jit, full


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
        sys.exit("bench_augment: no GPU; this measurement has no CPU form")
    dev = torch.device("cuda")
    imgs, mats, flips, jit, full = inputs()
    desc = np.zeros(B, T._CROP_DTYPE)
    for i, im in enumerate(imgs):
        desc[i] = (i * im.size, SRC_H, SRC_W, int(flips[i]), 0, T.invert_affine(mats[i]))
    SETS = 4
    src0 = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    dtab = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    cropper = T.DeviceCropper((W, H), "cpu")           # only its table builders are used here
    jt, _ = cropper._jitter_table(jit, B)
    to_dev = lambda tab: torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    jon = to_dev(jt)
    a_full = to_dev(cropper._augment_table(full, jt, B)[0])
    a_noblur = to_dev(cropper._augment_table([{"noise": d["noise"]} for d in full], jt, B)[0])
    only_jitter = np.zeros(B, T._AUG_DTYPE)
    only_jitter["jit"] = jt
    a_jitter, a_off = to_dev(only_jitter), torch.zeros_like(a_full)
    ws_bytes = _lib.lib.pk_affine_crop_augment_ws_bytes(B, W, H)
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

    def table_of(entry, table):
        return rotating(getattr(_lib.lib, entry),
                        [(s.data_ptr(), dtab.data_ptr(), table.data_ptr(), B, W, H, o32.data_ptr(), o16.data_ptr(), mean, std, ws.data_ptr(), ws.numel(), st)
                         for s, o32, o16, ws in sets], entry)

    aug, jitter = "pk_affine_crop_augment_normalize", "pk_affine_crop_jitter_normalize"
    variants = {"plain": plain_of(_lib.lib), "jitter": table_of(jitter, jon), "augment": table_of(aug, a_full), "blur_off": table_of(aug, a_noblur)}
    guards = {"plain": {"augment entry with every stage off": table_of(aug, a_off)}, "jitter": {"augment entry with only the jitter on": table_of(aug, a_jitter)}}
    if args.baseline_lib:
        other = ctypes.CDLL(os.path.abspath(args.baseline_lib))
        other.pk_affine_crop_normalize.argtypes = _lib.declared_symbols()["pk_affine_crop_normalize"][1]
        other.pk_affine_crop_normalize.restype = ctypes.c_int
        variants["baseline"] = guards["plain"]["baseline build"] = plain_of(other)
    # the outputs that must agree, before anything is timed
    for against, checks in guards.items():
        for _ in range(SETS):
            variants[against]()
        ref = [(o32.clone(), o16.clone()) for _, o32, o16, _ in sets]
        for name, fn in checks.items():
            for _, o32, o16, _ in sets:
                o32.zero_(), o16.zero_()
            for _ in range(SETS):
                fn()
            for (r32, r16), (_, o32, o16, _) in zip(ref, sets):
                assert torch.equal(o32, r32) and torch.equal(o16, r16), f"{name} does not reproduce the {against} crop"
    variants["augment"]()
    assert not torch.equal(sets[1][1], ref[1][0]), "the augment path left the crop unchanged"
    for fn in variants.values():                     # warm-up: code objects, clocks
        window(fn, 50)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "workload": f"{B} x {SRC_W}x{SRC_H} -> {W}x{H}, fp32 NCHW + bf16 NHWC-8",
           "repeats": args.repeats, "iters": args.iters, "buffer_sets": SETS, "kernel_us": {}}
    for k, v in times.items():
        med = statistics.median(v)
        res["kernel_us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        print(f"{k:9s} {med:8.2f} us per call (min {min(v):.2f}, max {max(v):.2f})", flush=True)
    med = lambda k: res["kernel_us"][k]["median"]
    res["jitter_over_plain"], res["augment_over_plain"] = round(med("jitter") / med("plain"), 3), round(med("augment") / med("plain"), 3)
    line = f"jitter / plain {res['jitter_over_plain']:.3f}   augment / plain {res['augment_over_plain']:.3f}"
    if "baseline" in res["kernel_us"]:
        for k in ("plain", "jitter", "augment"):
            res[f"{k}_over_baseline"] = round(med(k) / med("baseline"), 3)
            line += f"   {k} / baseline {res[f'{k}_over_baseline']:.3f}"
    print(line, flush=True)

    # the whole DeviceCropper call: staging + one copy + launches
    crop = T.DeviceCropper((W, H), dev)
    res["cropper_ms"] = {}
    for name, kw in (("plain", {}), ("jitter", {"jitter": jit}), ("augment", {"jitter": jit, "augment": full})):
        for _ in range(5):
            crop(imgs, mats, flips, **kw)
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            crop(imgs, mats, flips, **kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        m = statistics.median(ts)
        res["cropper_ms"][name] = {"median": round(m, 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "img_per_s": round(B / m * 1e3)}
        print(f"DeviceCropper {name:7s} {m:.3f} ms per {B} images (min {min(ts):.3f}, max {max(ts):.3f}) = {B / m * 1e3:.0f} img/s", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
