#!/usr/bin/env python3
"""Cost of the limb-kinematics kernels (run on the GPU box, under a time limit of its own).

    timeout -k 10 600 python scripts/bench_kinematics.py [--repeats 10] [--iters 20]

Workloads: (S, T, K) = (1, 18000, 17), ten minutes of one infant at 30 frames a second, with the 8 angles of COCO_ANGLES, and (64, 900, 13),
64 clips of half a minute of a 13-joint layout (COCO without eyes and ears: joint j of COCO is joint j - 4), with the same 8 angles under
those numbers; with confidences.  The series of each is (S, T, 8 + K): the angles, then the joint speeds.
  * pk_joint_angles and pk_joint_speeds on the trajectories;
  * pk_series_stats on the series;
  * pk_series_xcorr (both launches) over the 4 left/right pairs of angles and the left/right pairs of joint speeds, max_lag 30 (61 lags);
  * pk_sample_entropy (both launches), m = 2, tol = 0.2 sd of each series.
Kernels only (the C entries called directly into preallocated outputs), device-resident inputs, HIP events around `iters` back-to-back
calls, `repeats` windows per variant with the variants ALTERNATING inside every repeat; median and min .. max of the per-call time.  Warm
numbers: the inputs stay in the caches between calls.  Before anything is timed every kernel is checked against its numpy restatement
(tests/kinematics_np.py) -- the entropy only on the first HOST_T frames, because the restatement holds all pairs at once -- and the
restatement is timed on the host of the same box (best of 3) for scale, the entropy again only at HOST_T frames.  Prints readable lines and
one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import kinematics_np as knp  # noqa: E402
from bench_motion import entry, host_ms, trajectories, window  # noqa: E402
from infantposeestimation_gaussianbias_amd import hipops  # noqa: E402

SHAPES = [(1, 18000, 17), (64, 900, 13)]
COCO_TRIPLES = list(knp.COCO_ANGLES.values())
TRIPLES = {17: COCO_TRIPLES, 13: [tuple(j - 4 for j in t) for t in COCO_TRIPLES]}
FLIP = {17: [(j, j + 1) for j in range(1, 17, 2)], 13: [(j, j + 1) for j in range(1, 13, 2)]}
MAX_LAG, M, R, HOST_T = 30, 2, 0.2, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kinematics: no GPU; this measurement has no CPU form")
    dev = torch.device("cuda")
    variants, host, checks = {}, {}, {}
    for S, T, K in SHAPES:
        c, conf = trajectories(S, T, K, S + T)
        dc, dconf = torch.from_numpy(c).to(dev), torch.from_numpy(conf).to(dev)
        tag, tri, A = f"{S}x{T}x{K}", TRIPLES[K], len(TRIPLES[K])
        pairs = [(2 * i, 2 * i + 1) for i in range(A // 2)] + [(A + a, A + b) for a, b in FLIP[K]]
        Q, P, NL = A + K, len(pairs), 2 * MAX_LAG + 1
        # ---- checks against the restatement
        ang, spd = hipops.joint_angles(dc, dconf, 0.3, tri), hipops.joint_speeds(dc, dconf, 0.3)
        want_a, want_s = knp.joint_angles(c, conf, 0.3, tri), knp.joint_speeds(c, conf, 0.3)
        assert np.array_equal(np.isnan(ang.cpu().numpy()), np.isnan(want_a)) and np.array_equal(np.isnan(spd.cpu().numpy()), np.isnan(want_s)), tag
        a_share = float(np.nanmax(np.abs(ang.cpu().numpy() - want_a))) / (16 * 2.0 ** -52 * np.pi)
        series = torch.cat([ang, spd], 2).contiguous()
        x = series.cpu().numpy()
        stats = hipops.series_stats(series)
        st, want_st = stats.cpu().numpy(), knp.series_stats(x)
        n = want_st[..., 0]
        assert all(np.array_equal(st[..., i], want_st[..., i]) for i in (0, 1, 2, 6, 7)), tag
        sum_abs = np.abs(np.where(np.isfinite(x), x, 0.0)).sum(1)
        m_share = float((np.abs(st[..., 3] - want_st[..., 3]) / ((n + 16) * 2.0 ** -52 * sum_abs / np.maximum(n, 1))).max())
        corr, count, _ = hipops.series_xcorr(series, pairs, MAX_LAG)
        want_r, want_n = knp.xcorr(x, pairs, MAX_LAG)
        assert np.array_equal(count.cpu().numpy(), want_n), tag
        r_share = float((np.abs(corr.cpu().numpy() - want_r) / ((want_n + 16) * 2.0 ** -50)).max())
        tol = (stats[..., 4] * R).contiguous()
        head = series[:, :HOST_T].contiguous()
        tol_head = (hipops.series_stats(head)[..., 4] * R).contiguous()
        got_e = hipops.sample_entropy_counts(head[:2], tol_head[:2].contiguous(), M).cpu().numpy()
        assert np.array_equal(got_e, knp.sample_entropy_counts(x[:2, :HOST_T], tol_head[:2].cpu().numpy(), M)), tag
        assert a_share <= 1.0 and m_share <= 1.0 and r_share <= 1.0, (tag, a_share, m_share, r_share)
        checks[tag] = {"angle_err_share_of_bound": a_share, "mean_err_share_of_bound": m_share, "xcorr_err_share_of_bound": r_share}
        # ---- the timed calls
        d_tri = torch.from_numpy(np.asarray(tri, np.int32)).to(dev)
        d_pairs = torch.from_numpy(np.asarray(pairs, np.int32)).to(dev)
        o_ang = torch.empty(S, T, A, dtype=torch.float64, device=dev)
        o_spd = torch.empty(S, T, K, dtype=torch.float64, device=dev)
        o_st = torch.empty(S, Q, 8, dtype=torch.float64, device=dev)
        o_r = torch.empty(S, P, NL, dtype=torch.float64, device=dev)
        o_n = torch.empty(S, P, NL, dtype=torch.int32, device=dev)
        o_sum = torch.empty(S, P, 4, dtype=torch.float64, device=dev)
        tiles = hipops.sample_entropy_tiles(T, M)
        ws = torch.empty(S * Q * tiles, 2, dtype=torch.int64, device=dev)
        o_e = torch.empty(S, Q, 3, dtype=torch.int64, device=dev)
        variants[f"joint_angles {tag} {A} angles"] = entry("pk_joint_angles", dc, dconf, d_tri, o_ang, S, T, K, A, 0.3)
        variants[f"joint_speeds {tag}"] = entry("pk_joint_speeds", dc, dconf, o_spd, S, T, K, 0.3)
        variants[f"series_stats {tag} Q={Q}"] = entry("pk_series_stats", series, o_st, S, T, Q)
        variants[f"series_xcorr {tag} P={P} L={MAX_LAG}"] = entry("pk_series_xcorr", series, d_pairs, o_r, o_n, o_sum, S, T, Q, P, MAX_LAG, 2)
        variants[f"sample_entropy {tag} Q={Q} m={M} ({tiles} tiles each)"] = entry("pk_sample_entropy", series, tol, ws, o_e, S, T, Q, M)
        host[f"joint_angles {tag} {A} angles"] = host_ms(lambda: knp.joint_angles(c, conf, 0.3, tri))
        host[f"joint_speeds {tag}"] = host_ms(lambda: knp.joint_speeds(c, conf, 0.3))
        host[f"series_stats {tag} Q={Q}"] = host_ms(lambda: knp.series_stats(x))
        host[f"series_xcorr {tag} P={P} L={MAX_LAG}"] = host_ms(lambda: knp.xcorr(x, pairs, MAX_LAG))
        xh, th = x[:1, :HOST_T], tol_head[:1].cpu().numpy()
        host[f"sample_entropy {tag} Q={Q} m={M} ({tiles} tiles each)"] = host_ms(lambda: knp.sample_entropy_counts(xh, th, M))

    for fn in variants.values():                     # warm-up: code objects, clocks
        window(fn, 5)
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(window(fn, args.iters))
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "iters": args.iters, "checks": checks, "call_us": {},
           "host_numpy_ms": {k: round(v, 3) for k, v in host.items()}, "host_entropy_frames": HOST_T}
    for k, v in times.items():
        med = statistics.median(v)
        res["call_us"][k] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        note = f" (ONE sequence of {HOST_T} frames)" if k.startswith("sample_entropy") else ""
        print(f"{k:58s} {med:10.2f} us per call (min {min(v):.2f}, max {max(v):.2f})   numpy on the host {host[k]:9.3f} ms{note}", flush=True)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
