#!/usr/bin/env python3
"""Time pose rescoring + OKS-NMS on the device (pk_pose_rescore + pk_oks_nms through hipops, csrc/pk_nms.hip) against the numpy restatement
the tests use (tests/oks_nms_np.py) on a COCO-val-sized set: 5 000 images x 20 poses of 17 keypoints (the test generator: clusters of
four jittered copies of a base pose), hard NMS at 0.9 and soft NMS at 0.9 with max_dets 20.  The device figure is a host clock around
rescore + NMS that ends in a synchronise, inputs already on the device (what COCOEvaluator.suppress launches; its host bookkeeping and
the upload are reported separately as `with_upload_s`).  Warm-up first, then `--repeats` repeats; the results of both implementations
are compared.  Prints one JSON line.

    python scripts/bench_oks_nms.py [--images 5000] [--poses 20] [--repeats 20] [--out FILE]
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

import oks_nms_np as onp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from infantposeestimation_gaussianbias_amd import hipops
    if not torch.cuda.is_available():
        raise SystemExit("bench_oks_nms: no GPU (the kernels have no CPU path)")
    kpt, area, _, off, vars_ = onp.make_batch((args.poses,) * args.images, 17, 0, tie=False)
    box = np.random.default_rng(1).uniform(0.05, 1.0, kpt.shape[0])
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"images": args.images, "poses_per_image": args.poses, "keypoints": 17, "repeats": args.repeats}
    for name, soft in (("hard_0.9", False), ("soft_0.9_max20", True)):
        def device_run(k, a, b, v):
            score = hipops.pose_rescore(k, b, 0.2)
            return score, hipops.oks_nms(k, a, score, off, v, 0.9, 0.2, soft, 20)
        k_d, a_d, b_d, v_d = up(kpt), up(area), up(box), up(vars_)
        for _ in range(3):                                        # warm-up: code objects, allocator
            device_run(k_d, a_d, b_d, v_d)
        torch.cuda.synchronize()
        resident, uploaded = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            score, got = device_run(k_d, a_d, b_d, v_d)
            torch.cuda.synchronize()
            resident.append(time.perf_counter() - t0)
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            _, res = device_run(up(kpt), up(area), up(box), up(vars_))
            host = [r.cpu() for r in res]                         # device->host copies: synchronised
            uploaded.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        score_np = onp.rescore_np(kpt, box, 0.2)
        want = onp.oks_nms_np(kpt, area, score_np, off, vars_, 0.9, 0.2, soft, 20)
        ref_s = time.perf_counter() - t0
        keep, n_keep, order, out_score = (g.cpu().numpy() for g in got)
        out[name] = {"device_s_median": float(np.median(resident)), "device_s_min": float(np.min(resident)), "device_s_max": float(np.max(resident)),
                     "with_upload_s_median": float(np.median(uploaded)), "numpy_restatement_s": round(ref_s, 2),
                     "kept": int(n_keep.sum()), "of": int(kpt.shape[0]), "restatement_margin": float(want[4]),
                     "same_keep": bool(np.array_equal(keep, want[0])), "same_order": bool(np.array_equal(order, want[2])),
                     "max_rel_score_diff": float((np.abs(out_score - want[3]) / np.maximum(np.abs(want[3]), 1e-300)).max())}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
