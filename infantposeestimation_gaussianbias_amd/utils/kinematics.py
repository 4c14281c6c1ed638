"""Limb kinematics of one pose trajectory (DESIGN.md "Limb kinematics"): joint angles, inter-limb coordination and movement complexity, the
three quantities a quantitative general-movement assessment adds to amplitudes and frequencies.  The reference prints an asymmetry ratio
(examples/quick_start.py:242-249) and stops; the arithmetic is this project's own specification.

Everything is computed by the kernels of csrc/pk_kinematics.hip on the device, where `predict_sequence` leaves the trajectory; what is left
on the host is naming, unit conversion (radians -> degrees, frames -> seconds) and -ln(A / B) of two integers.  Numpy input is uploaded;
without a GPU these raise like every other op."""
import math
from typing import Dict, Optional

import numpy as np

from .metrics import _sequence_in

# name -> joints (a, b, c) of the 17-joint COCO layout: the interior angle at b between the rays to a and to c
COCO_ANGLES = {
    "left_elbow": (5, 7, 9), "right_elbow": (6, 8, 10), "left_shoulder": (7, 5, 11), "right_shoulder": (8, 6, 12),
    "left_hip": (5, 11, 13), "right_hip": (6, 12, 14), "left_knee": (11, 13, 15), "right_knee": (12, 14, 16),
}
DEFAULT_MAX_LAG = 30                                              # frames, when no frame rate says what a second is


def _angle_table(num_joints: int, angles):
    """`angles` (None or a mapping name -> (a, b, c)) -> names, triples for a layout of `num_joints` joints.  ValueError for a layout
    without a default table, an empty table or a triple that is not three joints of the layout with the middle one distinct."""
    if angles is None:
        if num_joints != 17:
            raise ValueError(f"joint angles: a layout of {num_joints} joints has no default angle table (COCO_ANGLES names the 17-joint "
                             "layout); pass angles={name: (a, b, c)}")
        angles = COCO_ANGLES
    from ..configs.config import check_joint_angles
    table = check_joint_angles(angles, "angles", num_joints)
    return list(table), [table[n] for n in table]


def _check_shape(seq):
    shape = tuple(seq.shape)
    if len(shape) != 3 or shape[-1] != 2:
        raise ValueError(f"sequence: expected (T, K, 2), got {shape}")
    return shape


def joint_angle_series(keypoints_sequence, confidence=None, min_confidence: float = 0.3, angles=None):
    """(T,K,2) trajectory -> (T,A) float64 joint angles in radians, in [0, pi]: the unsigned interior angle at the middle joint of each
    triple of `angles` (a mapping name -> (a, b, c); None: `COCO_ANGLES` for 17 joints), NaN where one of the three joints is not finite,
    is below `min_confidence`, or coincides with the middle one (pk_joint_angles).  numpy in -> numpy out, device in -> device out."""
    from .. import hipops
    shape = _check_shape(keypoints_sequence)
    _, triples = _angle_table(shape[1], angles)
    coords, conf, as_numpy = _sequence_in(keypoints_sequence, confidence)
    out = hipops.joint_angles(coords, conf, min_confidence, triples)[0]
    return out.cpu().numpy() if as_numpy else out


def _series_in(series, name):
    """(T,) or (T,Q) numpy array / device tensor -> float64 device tensor (1,T,Q), came_as_numpy, was_one_dimensional."""
    import torch
    from .. import _lib
    if len(tuple(series.shape)) not in (1, 2):
        raise ValueError(f"{name}: expected (T,) or (T, Q), got {tuple(series.shape)}")
    as_numpy = not isinstance(series, torch.Tensor)
    if as_numpy:
        if not torch.cuda.is_available():
            raise _lib.PoseKernelError(f"{name}: expected a CUDA(HIP) device; the kernels have no CPU implementation")
        series = torch.from_numpy(np.ascontiguousarray(np.asarray(series), dtype=np.float64)).to(torch.device("cuda", torch.cuda.current_device()))
    elif not series.is_cuda:
        raise _lib.PoseKernelError(f"{name}: expected a CUDA(HIP) tensor or a numpy array; the kernels have no CPU implementation")
    flat = series.dim() == 1
    series = series.double()
    return (series[:, None] if flat else series)[None].contiguous(), as_numpy, flat


def _coordination(summary_row, fps) -> Dict:
    lag = int(summary_row[1])
    return {"r0": float(summary_row[0]), "peak_r": float(summary_row[2]), "peak_lag": lag,
            "peak_lag_s": None if fps is None else lag / float(fps), "pairs_used": int(summary_row[3])}


def limb_coordination(series_a, series_b, max_lag: int, fps: Optional[float] = None) -> Dict:
    """Normalised cross-correlation of two (T,) series (NaN = no value) over the lags -max_lag .. max_lag (pk_series_xcorr): Pearson's r of
    a[t] against b[t + lag] over the frames where both are valid, so a POSITIVE peak lag says that `series_a` leads.  ->
      lags (2L+1,) frames, r (2L+1,) and pairs (2L+1,) int32: numpy in -> numpy out, device in -> device out;
      r0, peak_r, peak_lag (frames), peak_lag_s (with `fps`, else None), pairs_used: over the lags with at least 2 pairs."""
    import torch
    from .. import hipops
    from ..configs.config import check_kinematics
    L = check_kinematics(max_lag=max_lag, what=("max_lag", "m", "r"))["max_lag"]
    if tuple(series_a.shape) != tuple(series_b.shape) or len(tuple(series_a.shape)) != 1:
        raise ValueError(f"limb_coordination: expected two series of one length (T,), got {tuple(series_a.shape)} and {tuple(series_b.shape)}")
    a, as_numpy, _ = _series_in(series_a, "series_a")
    b, _, _ = _series_in(series_b, "series_b")
    corr, count, summary = hipops.series_xcorr(torch.cat([a, b.to(a.device)], 2), [(0, 1)], L)
    out = _coordination(summary[0, 0].cpu().numpy(), fps)
    lags = np.arange(-L, L + 1)
    out["lags"] = lags if as_numpy else torch.from_numpy(lags).to(a.device)
    out["r"], out["pairs"] = (corr[0, 0].cpu().numpy(), count[0, 0].cpu().numpy()) if as_numpy else (corr[0, 0], count[0, 0])
    return out


def _entropy_value(row) -> Optional[float]:
    """(|W|, B, A) -> SampEn = -ln(A / B), None when A or B is 0 (no pair of templates matches: the entropy is not defined)."""
    B, A = int(row[1]), int(row[2])
    return None if A == 0 or B == 0 else 0.0 - math.log(A / B)    # 0.0, not -0.0, when every pair matches


def sample_entropy(series, m: int = 2, r: float = 0.2):
    """Sample entropy SampEn(m, r) of a (T,) series, or of each column of a (T,Q) one (NaN = no value): -ln(A / B), B and A the pairs of
    valid templates that match within r x (the series' population sd) over m and m + 1 elements (pk_series_stats for the sd, one float64
    multiply on the device for the tolerance, pk_sample_entropy for the counts).  -> float or None (no matching pair), a list for (T,Q)."""
    from .. import hipops
    from ..configs.config import check_kinematics
    m, r = check_kinematics(entropy=(m, r), what=("max_lag", "m", "r"))["entropy"]
    x, _, flat = _series_in(series, "series")
    tol = hipops.series_stats(x)[..., 4] * r
    counts = hipops.sample_entropy_counts(x, tol.contiguous(), m)[0].cpu().numpy()
    values = [_entropy_value(row) for row in counts]
    return values[0] if flat else values


def kinematics_report(keypoints_sequence, confidence=None, flip_pairs=(), angles=None, min_confidence: float = 0.3,
                      fps: Optional[float] = None, max_lag: Optional[int] = None, entropy=(2, 0.2)) -> Dict:
    """JSON-serialisable limb kinematics of one (T,K,2) trajectory (numpy array or device tensor).
      angles        per named angle (`angles`: name -> (a, b, c); None: `COCO_ANGLES` for 17 joints): joints, valid_fraction, min_deg, max_deg,
                    range_deg, mean_deg, sd_deg, angular_path_deg, mean_angular_speed and max_angular_speed (deg / frame, or deg / s with
                    `fps`), sample_entropy (None where no pair of templates matches)
      joints        per joint: speed_entropy, the sample entropy of its speed series |p[t+1] - p[t]|
      coordination  per pair of angles named left_X / right_X and per (left, right) of `flip_pairs` (their speed series): r0, peak_r, peak_lag
                    (frames; positive: the left side leads), peak_lag_s (with `fps`), pairs_used
    max_lag: lags searched on both sides (None: one second, round(fps), with `fps`, else 30 frames; capped at T - 2).  entropy: (m, r),
    template length and tolerance as a share of each series' standard deviation.
    One (T, A + K) series on the device (angles, then speeds), one statistics, one cross-correlation and one entropy call; the (A + K, 8)
    statistics, the (P, 4) correlation summary and the (A + K, 3) entropy counts are what comes back."""
    import torch
    from .. import hipops
    from ..configs.config import check_kinematics
    T, K, _ = _check_shape(keypoints_sequence)
    names, triples = _angle_table(K, angles)
    checked = check_kinematics(max_lag=max_lag, entropy=entropy, what=("max_lag", "entropy m", "entropy r"))
    m, r = checked["entropy"]
    if fps is not None and not (math.isfinite(float(fps)) and float(fps) > 0):
        raise ValueError(f"fps must be a positive number, got {fps!r}")
    L = checked["max_lag"] if max_lag is not None else (DEFAULT_MAX_LAG if fps is None else int(round(float(fps))))
    L = max(0, min(L, T - 2, hipops.KIN_MAX_LAG))
    A = len(names)
    pairs, labels = [], []
    for i, name in enumerate(names):
        if name.startswith("left_") and "right_" + name[5:] in names:
            pairs.append((i, names.index("right_" + name[5:])))
            labels.append({"kind": "angle", "left": name, "right": "right_" + name[5:]})
    for left, right in flip_pairs:
        if not (0 <= int(left) < K and 0 <= int(right) < K):
            raise ValueError(f"flip_pairs: ({left}, {right}) names a joint outside 0 to {K - 1}")
        pairs.append((A + int(left), A + int(right)))
        labels.append({"kind": "joint_speed", "left": int(left), "right": int(right)})

    coords, conf, _ = _sequence_in(keypoints_sequence, confidence)
    series = torch.cat([hipops.joint_angles(coords, conf, min_confidence, triples), hipops.joint_speeds(coords, conf, min_confidence)], 2)
    stats_dev = hipops.series_stats(series)
    counts = hipops.sample_entropy_counts(series, (stats_dev[..., 4] * r).contiguous(), m)[0].cpu().numpy()
    stats = stats_dev[0].cpu().numpy()
    summary = hipops.series_xcorr(series, pairs, L)[2][0].cpu().numpy() if pairs and T > 0 else np.zeros((len(pairs), 4))

    rate, deg = 1.0 if fps is None else float(fps), 180.0 / math.pi
    angle_rows = []
    for i, name in enumerate(names):
        st = stats[i]
        steps = float(st[6])
        angle_rows.append({"name": name, "joints": [int(j) for j in triples[i]], "valid_fraction": float(st[0]) / T if T > 0 else 0.0,
                           "min_deg": float(st[1]) * deg, "max_deg": float(st[2]) * deg, "range_deg": (float(st[2]) - float(st[1])) * deg,
                           "mean_deg": float(st[3]) * deg, "sd_deg": float(st[4]) * deg, "angular_path_deg": float(st[5]) * deg,
                           "mean_angular_speed": float(st[5]) * deg / steps * rate if steps > 0 else 0.0,
                           "max_angular_speed": float(st[7]) * deg * rate, "sample_entropy": _entropy_value(counts[i])})
    return {"num_frames": T, "fps": None if fps is None else float(fps), "angular_speed_unit": "deg/frame" if fps is None else "deg/s",
            "max_lag": L, "entropy": {"m": m, "r": r}, "angles": angle_rows,
            "joints": [{"joint": k, "speed_entropy": _entropy_value(counts[A + k])} for k in range(K)],
            "coordination": [dict(label, **_coordination(summary[p], fps)) for p, label in enumerate(labels)]}
