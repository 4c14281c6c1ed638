"""Movement analysis and PCK without a GPU: the numpy restatements (tests/motion_np.py) against closed forms, the bin rule against
np.histogram2d, the PCK decision at exact ties, the legacy-yaml mapping of the EVAL / TEMPORAL / CLINICAL blocks, the three new entries in
the header, and the op layer's shape checks.  The library functions themselves raise without a device, so nothing here calls them past
their argument checks."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import motion_np as mnp
from conftest import GOLDEN

F32 = np.float32


# ------------------------------------------------------------------------------------------------ restatement against closed forms
def test_circle_has_the_range_of_its_diameter_and_the_path_of_its_polygon():
    """200 frames at the corners of the regular 200-gon inscribed in a circle of radius 30, in float64 (the restatement widens whatever
    it is given): the corners at 0, 90, 180 and 270 degrees are among them, so each axis ranges over the diameter; the 199 steps are 199
    of the polygon's 200 equal sides, i.e. its perimeter less the closing side."""
    T, R = 200, 30.0
    a = 2 * np.pi * np.arange(T) / T
    pts = np.stack([320 + R * np.cos(a), 240 + R * np.sin(a)], -1)
    st = mnp.motion_stats(pts[None, :, None, :])[0, 0]
    side = 2 * R * np.sin(np.pi / T)
    assert st[0] == T and st[7] == T - 1 and st[10] == T - 2
    assert abs((st[2] - st[1]) - 60.0) <= 1e-9 and abs((st[4] - st[3]) - 60.0) <= 1e-9
    assert abs(st[5] - 60.0 * np.sqrt(2.0)) <= 1e-9
    assert abs(st[6] - (T * side - side)) <= 1e-9
    assert abs(st[8] - side) <= 1e-9
    # second difference of a uniformly sampled circle: |p[t+1] - 2 p[t] + p[t-1]| = R (2 - 2 cos(2 pi / T)) at every corner
    assert abs(st[9] - (T - 2) * R * (2 - 2 * np.cos(2 * np.pi / T))) <= 1e-9


def test_constant_velocity_has_no_acceleration():
    T, v = 500, np.array([0.75, -0.5])                            # exactly representable steps: every point is exact in float32
    pts = (np.array([100.0, 400.0]) + np.arange(T)[:, None] * v).astype(F32)
    st = mnp.motion_stats(pts[None, :, None, :])[0, 0]
    assert st[10] == T - 2
    assert st[9] <= T * 2.0 ** -40 * np.linalg.norm(v)
    assert abs(st[6] - (T - 1) * np.linalg.norm(v)) <= (T + 16) * 2.0 ** -52 * st[6]
    assert abs(st[8] - np.linalg.norm(v)) <= 4 * 2.0 ** -52


def test_quick_start_wrists_are_symmetric():
    seq = mnp.quick_start_wrists()
    st = mnp.motion_stats(seq[None])[0]
    assert mnp.asymmetry_ratio(st[0, 5], st[1, 5]) < 0.2
    # the reference's own figure, on the x ranges (examples/quick_start.py:239-242)
    rl, rr = np.ptp(seq[:, 0, 0].astype(np.float64)), np.ptp(seq[:, 1, 0].astype(np.float64))
    assert abs(rl - rr) / max(rl, rr) < 0.2
    assert mnp.flag(st[0, 5]) is None and mnp.flag(st[1, 5]) is None and mnp.flag(1.0) == "low" and mnp.flag(250.0) == "high"
    assert mnp.asymmetry_ratio(0.0, 0.0) == 0.0


def test_validity_rules_of_the_restatement():
    """One joint, five frames, frame 2 dropped: 4 valid frames, the steps 0->1 and 3->4 only, no triple; a (T,K) confidence exactly at
    the threshold counts."""
    pts = np.array([[0, 0], [3, 4], [100, 100], [6, 8], [6, 8]], F32)[None, :, None, :]
    conf = np.array([0.9, F32(0.3), 0.1, 0.9, 0.9], F32)[None, :, None]
    st = mnp.motion_stats(pts, conf, 0.3)[0, 0]
    assert st.tolist() == [4, 0, 6, 0, 8, 10, 5, 2, 5, 0, 0]
    nan = pts.copy()
    nan[0, 2, 0, 1] = np.inf
    assert np.array_equal(mnp.motion_stats(nan)[0, 0], st)
    assert not mnp.motion_stats(np.full((1, 3, 1, 2), np.nan, F32)).any()


# ------------------------------------------------------------------------------------------------ bin rule
@pytest.mark.parametrize("W,H,nbx,nby", [(640, 480, 64, 48), (333, 217, 33, 21), (7, 5, 1, 1), (30, 20, 3, 2)])
def test_bin_rule_equals_histogram2d(W, H, nbx, nby):
    pts = mnp.edge_points(W, H, nbx, nby)
    assert np.isnan(pts).any() and np.isinf(pts).any() and (pts[:, 0] == F32(W)).any() and np.signbit(pts[pts == 0]).any()
    assert (pts[:, 0] == np.nextafter(F32(W), F32(np.inf))).any() and (pts[:, 0] == np.nextafter(F32(W), F32(0))).any()
    ex, ey = np.linspace(0, W, nbx + 1), np.linspace(0, H, nby + 1)
    allp = pts[None, :, None, :]
    got = mnp.position_histogram(allp, ex, ey)
    # np.histogram2d counts NaN and infinite samples in no bin when it is handed the edges; the rule here declares such frames invalid
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    assert np.array_equal(got[0, 0], np.histogram2d(x, y, bins=[ex, ey])[0].T) and got.sum() > 0
    # ... and the uniform-bin form the reference calls (visualization.py:248-252) on the finite points gives the same counts
    fin = np.isfinite(pts).all(-1)
    assert np.array_equal(got[0, 0], np.histogram2d(x[fin], y[fin], bins=[nbx, nby], range=[[0, W], [0, H]])[0].T)
    assert np.array_equal(mnp.histogram2d(allp, ex, ey), got)
    assert mnp.bin_index(np.nan, ex) == -1 and mnp.bin_index(np.inf, ex) == -1 and mnp.bin_index(-0.0, ex) == 0
    assert mnp.bin_index(float(W), ex) == nbx - 1 and mnp.bin_index(float(np.nextafter(F32(W), F32(np.inf))), ex) == -1


def test_bin_rule_on_uneven_edges():
    """The walk makes the rule exact for any ascending edges, however poor the linear guess."""
    e = np.array([0.0, 0.001, 0.002, 50.0, 99.0, 99.5, 100.0])
    g = np.random.default_rng(5)
    v = np.concatenate([e, g.random(500) * 100, g.random(100) * 0.003, [100.0, -1e-9, 100.0000001]])
    want = np.histogram(v, bins=e)[0]
    got = np.bincount([i for i in (mnp.bin_index(x, e) for x in v) if i >= 0], minlength=len(e) - 1)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ PCK at exact ties
def test_pck_restatement_decides_ties_as_hits_and_one_ulp_more_as_a_miss():
    r = mnp.TIE_THR * mnp.TIE_NORM
    rr = r * r
    d2_on = F32(4) * F32(4) + F32(0) * F32(0)
    d2_out = F32(4) * F32(4) + mnp.TIE_DY * mnp.TIE_DY
    assert rr.dtype == F32 and d2_on == rr and d2_out == np.nextafter(rr, F32(np.inf))
    pred = np.array([[[4, 0]], [[4, mnp.TIE_DY]], [[4, 0]], [[4, 0]], [[np.nan, 0]]], F32)
    gt = np.zeros((5, 1, 2), F32)
    vis, norm = np.array([[2], [1], [0], [1], [1]], F32), np.array([8, 8, 8, 0, 8], F32)
    correct, valid, err = mnp.pck(pred, gt, vis, norm, [0.5, 0.6])
    assert correct.tolist() == [[1], [2]] and valid.tolist() == [2]
    assert abs(err[0] - (0.5 + np.sqrt(float(d2_out)) / 8)) <= 4 * 2.0 ** -52
    # the builder plants the same two pairs
    p, g_, v, n, t = mnp.pck_case(257, 17, 6)
    c1, _, _ = mnp.pck(p[:2], g_[:2], v[:2], n[:2], t)
    hit0 = mnp.pck(p[:1], g_[:1], v[:1], n[:1], t)[0][0, 0]
    assert t[0] == mnp.TIE_THR and hit0 == 1 and c1[0, 0] == 1


# ------------------------------------------------------------------------------------------------ config
def test_yaml_mapping_of_the_eval_temporal_and_clinical_blocks(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.configs.config import Config
    fields = [f.name for f in dataclasses.fields(Config)]
    assert fields == ["data", "model", "train", "exp_name", "seed"]
    base = get_config()
    assert (base.eval_metrics, base.pck_threshold, base.min_keypoint_visibility, base.temporal, base.clinical) == (("AP",), 0.2, 0.3, None, None)
    pre = get_config(os.path.join(GOLDEN, "eval_blocks_preemie_optimized.yaml"))
    assert pre.eval_metrics == ("AP", "PCK", "temporal_consistency") and pre.pck_threshold == 0.2 and pre.min_keypoint_visibility == 0.3
    assert pre.temporal == (5, "gaussian")
    assert pre.clinical == {"min_movement": 5.0, "max_movement": 200.0, "alert_low": False, "alert_asymmetry": False}
    dft = get_config(os.path.join(GOLDEN, "eval_blocks_default.yaml"))
    assert dft.eval_metrics == ("AP", "PCK") and dft.pck_threshold == 0.2 and dft.temporal is None and dft.clinical is None
    # a loaded yaml does not leak into the class, and the dataclass surface is the reference's
    assert (Config.eval_metrics, Config.temporal, Config.clinical) == (("AP",), None, None)
    assert [f.name for f in dataclasses.fields(Config)] == fields and set(dataclasses.asdict(pre)) == set(fields)

    def y(text):
        p = tmp_path / "legacy.yaml"
        p.write_text(text)
        return str(p)

    with pytest.raises(ValueError, match="odd"):
        get_config(y("TEMPORAL:\n  ENABLED: true\n  WINDOW_SIZE: 4\n"))
    assert get_config(y("TEMPORAL:\n  ENABLED: false\n  WINDOW_SIZE: 4\n")).temporal is None
    assert get_config(y("TEMPORAL:\n  ENABLED: true\n  WINDOW_SIZE: 7\n  SMOOTHING_METHOD: uniform\n")).temporal == (7, "uniform")
    assert get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: false\n  MIN_MOVEMENT_THRESHOLD: 9\n")).clinical is None
    got = get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: true\n  MIN_MOVEMENT_THRESHOLD: 9\n  ALERT_ON_ASYMMETRY: true\n")).clinical
    assert got == {"min_movement": 9.0, "max_movement": 200.0, "alert_low": False, "alert_asymmetry": True}
    assert get_config(y("EVAL:\n  PCK_THRESHOLD: 0.5\n")).pck_threshold == 0.5 and get_config(y("")).eval_metrics == ("AP",)


# ------------------------------------------------------------------------------------------------ C-ABI and op layer
def test_the_three_entries_are_declared_and_check_their_arguments():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_pck", 12), ("pk_motion_stats", 8), ("pk_position_histogram", 12)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(_lib.lib, name)
    L, p = _lib.lib, 64                                           # a non-null pointer value that is never dereferenced: the checks refuse first
    assert L.pk_pck(p, p, p, p, p, p, p, p, 4, 3, 17, None) == -1 and b"thresholds" in L.pk_last_error_string()
    assert L.pk_pck(p, p, p, p, p, p, p, p, 4, 3, 0, None) == -1
    assert L.pk_pck(p, p, p, None, p, p, p, p, 4, 3, 1, None) == -1 and b"null pointer" in L.pk_last_error_string()
    assert L.pk_motion_stats(None, None, p, 1, 1, 1, 0.3, None) == -1 and L.pk_motion_stats(p, None, p, 1, 0, 1, 0.3, None) == -1
    assert L.pk_position_histogram(p, None, p, p, p, 1, 5, 1, 129, 128, 0.3, None) == -2
    assert b"larger bins" in L.pk_last_error_string()
    assert L.pk_position_histogram(p, None, p, p, p, 1, 5, 1, 0, 4, 0.3, None) == -1
    assert L.pk_position_histogram(p, None, None, p, p, 1, 5, 1, 4, 4, 0.3, None) == -1


def test_the_limits_of_the_analysis_entries_come_from_the_public_header():
    """The six limits that the library and the op layer both check: one #define each in include/posekernels.h, parsed by _lib, carried by
    the hipops names and printed by the entries that refuse a value beyond them (PCK, histogram, spectrum, rescoring / OKS-NMS)."""
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    want = {"PK_PCK_MAX_THR": 16, "PK_HIST_MAX_BINS": 16384, "PK_SPEC_MAX_BINS": 16384, "PK_SPEC_MAX_NFFT": 1073741824, "PK_NMS_MAX_K": 64,
            "PK_NMS_MAX_POSES": 1024}
    assert {k: _lib.CONSTANTS.get(k) for k in want} == want
    assert _lib.CONSTANTS == _lib.declared_constants() and _lib.CONSTANTS["PK_REDUCE_BLOCKS"] == 1024 and _lib.CONSTANTS["PK_OHKM_MAX_K"] == 256
    assert (hipops.PCK_MAX_THRESHOLDS, hipops.HIST_MAX_BINS, hipops.SPECTRUM_MAX_BINS, hipops.SPECTRUM_MAX_NFFT, hipops.OKS_NMS_MAX_K,
            hipops.OKS_NMS_MAX_POSES) == (16, 16384, 16384, 1073741824, 64, 1024)
    L, p = _lib.lib, 64                                           # a non-null pointer value that is never dereferenced: the checks refuse first
    err = lambda: L.pk_last_error_string().decode()
    assert L.pk_pck(p, p, p, p, p, p, p, p, 4, 3, 17, None) == -1 and err() == "pk_pck: 17 thresholds (1 to 16)"
    assert L.pk_position_histogram(p, None, p, p, p, 1, 5, 1, 128, 129, 0.3, None) == -2
    assert err() == "pk_position_histogram: 128 x 129 bins exceed the 16384 a workgroup keeps in LDS; take larger bins"
    assert L.pk_motion_spectrum(p, None, p, p, 1, 5, 1, 0.3, 1 << 20, 1, 16385, 0, None) == -1
    assert err() == "pk_motion_spectrum: 16385 bins (1 to 16384)"
    assert L.pk_motion_spectrum(p, None, p, p, 1, 5, 1, 0.3, (1 << 30) + 1, 1, 4, 0, None) == -1
    assert err() == "pk_motion_spectrum: transform length N=1073741825 (2 to 1073741824)"
    assert L.pk_pose_rescore(p, None, p, 3, 65, 0.2, None) == -1 and err() == "pk_pose_rescore: bad size (N 3, K 65; 1 <= K <= 64)"
    assert L.pk_oks_nms(p, p, p, p, p, p, p, p, p, 2, 65, 0.9, 0.2, 0, 20, None) == -1
    assert err() == "pk_oks_nms: bad size (n_img 2, K 65; 1 <= K <= 64)"
    # the poses of an image are device data: the op layer counts them on the host and refuses before any device work
    n, va = hipops.OKS_NMS_MAX_POSES + 1, torch.ones(17, dtype=torch.float64)
    with pytest.raises(_lib.PoseKernelError, match="image 0 holds 1025 poses; the kernel is built for at most 1024 per image"):
        hipops.oks_nms(torch.zeros(n, 17, 3, dtype=torch.float64), torch.ones(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64),
                       np.array([0, n], np.int32), va, 0.9)


def test_op_layer_refuses_mismatched_shapes_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z = torch.zeros
    acc = (z(2, 3, dtype=torch.int64), z(3, dtype=torch.int64), z(3, dtype=torch.float64))
    good = (z(4, 3, 2), z(4, 3, 2), z(4, 3), z(4), z(2))
    for i, bad in ((0, z(4, 3, 3)), (1, z(4, 2, 2)), (2, z(4, 4)), (3, z(5)), (4, z(17)), (4, z(0)), (4, z(2, 1))):
        args = list(good)
        args[i] = bad
        with pytest.raises(ValueError):
            hipops.pck_accumulate(*args, *acc)
    with pytest.raises(ValueError, match="accumulators"):
        hipops.pck_accumulate(*good, z(3, 3, dtype=torch.int64), acc[1], acc[2])
    with pytest.raises(ValueError, match="contiguous"):
        hipops.pck_accumulate(*good, z(3, 2, dtype=torch.int64).t(), acc[1], acc[2])
    for fn in (hipops.motion_stats, lambda c, conf=None: hipops.position_histogram(c, np.linspace(0, 1, 3), np.linspace(0, 1, 3), conf)):
        with pytest.raises(ValueError, match="coords"):
            fn(z(5, 3, 2))
        with pytest.raises(ValueError, match="conf"):
            fn(z(1, 5, 3, 2), z(1, 5, 4))
    with pytest.raises(ValueError, match="edges"):
        hipops.position_histogram(z(1, 5, 3, 2), np.zeros(1), np.linspace(0, 1, 3))
    # right shapes on the host: refused as host tensors (no CPU implementation), still without a launch
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    with pytest.raises(PoseKernelError):
        hipops.motion_stats(z(1, 5, 3, 2))
    with pytest.raises(PoseKernelError):
        hipops.pck_accumulate(*good, *acc)


def test_public_functions_check_shapes_and_have_no_host_path():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    seq = mnp.quick_start_wrists(20)
    with pytest.raises(ValueError, match="sequence"):
        utils.calculate_movement_amplitude(seq[0])
    with pytest.raises(ValueError, match="confidence"):
        utils.calculate_temporal_consistency(seq, np.ones((20, 3), F32))
    with pytest.raises(ValueError, match="bin_size"):
        utils.movement_heatmap(seq, (5, 5), bin_size=10)
    with pytest.raises(ValueError, match="thresholds"):
        utils.PCKAccumulator(17, ())
    if not torch.cuda.is_available():
        for call in (lambda: utils.calculate_movement_amplitude(seq), lambda: utils.movement_report(seq),
                     lambda: utils.movement_heatmap(seq, (480, 640)), lambda: utils.calculate_temporal_consistency(torch.from_numpy(seq)),
                     lambda: utils.calculate_pck(np.zeros((2, 3, 2)), np.zeros((2, 3, 2)), np.ones((2, 3)), np.ones(2))):
            with pytest.raises(PoseKernelError):
                call()
