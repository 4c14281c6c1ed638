#!/usr/bin/env python3
"""Time COCOKeypointEval.evaluate (HIP kernels of csrc/pk_eval.hip + host bookkeeping) against the numpy restatement of COCOeval used by
the tests (tests/cocoeval_np.py) on a synthetic COCO-val-sized set: 5 000 images, ~6 400 ground truths (Poisson, mean 1.28 per image),
ground truths sitting 450 px apart, ~5 % crowd and ~5 % num_keypoints 0.  Two detection sets: one noisy copy per ground truth (~6 400), and 10-30
detections per image (~100 k; noisy copies plus false positives).  Prints one JSON line; the stats of both implementations are compared.

    python scripts/bench_coco_eval.py [--images 5000] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coco_cases as cc  # noqa: E402
import cocoeval_np  # noqa: E402


def make_set(n_img, dense, seed=0):
    rng = np.random.default_rng(seed)
    anns, recs, aid = [], [], 1
    for img in range(1, n_img + 1):
        gts = []
        for j in range(min(int(rng.poisson(1.28)), 20)):
            side = float(np.exp(rng.uniform(np.log(15), np.log(260))))
            kp = cc.pose(17, 450.0 * (j % 10), 450.0 * (j // 10), side, rng)
            kp[rng.random(17) < 0.15, 2] = 0
            extra = {'iscrowd': 1} if rng.random() < 0.05 else ({'num_keypoints': 0} if rng.random() < 0.05 else {})
            anns.append(cc.gt_ann(aid, img, kp, side * side * 0.8, bbox=[450.0 * (j % 10), 450.0 * (j // 10), side, side], **extra))
            gts.append((kp, side))
            aid += 1
        if not dense:
            picks = [g for g in gts]
        else:
            picks = [gts[int(rng.integers(len(gts)))] if gts and rng.random() < 0.5 else None for _ in range(int(rng.integers(10, 31)))]
        for g in picks:
            if g is None:
                det = cc.pose(17, rng.uniform(0, 4000), rng.uniform(0, 1000), float(rng.uniform(10, 250)), rng)
            else:
                det = g[0].copy()
                det[:, :2] += rng.normal(0, g[1] * rng.uniform(0.01, 0.2), (17, 2))
            recs.append(cc.rec(img, det, float(rng.uniform(0, 1))))
    return cc.dataset(list(range(1, n_img + 1)), anns), recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import COCOKeypointEval
    if not torch.cuda.is_available():
        raise SystemExit("bench_coco_eval: no GPU (the native evaluator has no CPU path)")
    out = {"images": args.images}
    for name, dense in (("one_per_gt", False), ("up_to_30_per_image", True)):
        ann, recs = make_set(args.images, dense)
        ev = COCOKeypointEval(ann, cc.COCO_SIGMAS)
        ev.evaluate(recs)                                     # warm-up: code objects, allocator
        native = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = COCOKeypointEval(ann, cc.COCO_SIGMAS)
            got = ev.evaluate(recs)                           # ends in device->host copies of the results: synchronised
            native.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = cocoeval_np.cocoeval(ann, recs, cc.COCO_SIGMAS)[0]
        ref_s = time.perf_counter() - t0
        out[name] = {"gts": len(ann["annotations"]), "dets": len(recs), "capped_dets": int(ev.slot_record.size),
                     "native_s": [round(v, 4) for v in native], "numpy_restatement_s": round(ref_s, 2),
                     "max_stat_diff": max(abs(got[k] - want[k]) for k in want), "AP": got["AP"], "AR": got["AR"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
