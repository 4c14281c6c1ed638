"""Movement analysis and PCK on the device: pk_motion_stats, pk_position_histogram and pk_pck against their numpy restatements
(tests/motion_np.py) and np.histogram2d at the sizes where the kernels change behaviour (no step, no triple, the 256-thread boundary, a
wrapped stride with a ragged tail, one bin, the largest LDS histogram), the public functions of utils/metrics.py, validate(pck_thresholds=)
and PoseInference.predict_sequence.

Tolerances.  Counts, minima and maxima are compared for equality.  The float64 sums (amplitude, path length, largest step, second-difference
sum, err_sum) are compared to relative (n + 16) 2^-52 with n the number of terms: both sides add at most n non-negative float64 terms, each
addition off by at most 2^-53 relative and nothing cancels; the 16 ulps cover the square roots and the last operations.  Derived, not
measured; every test prints what it saw."""
import functools
import json
import logging

import numpy as np
import pytest
import torch

import motion_np as mnp

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT_COLS, SUM_COLS = (0, 1, 2, 3, 4, 7, 10), (5, 6, 8, 9)


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached cases are read-only


def _rel(got, want):
    """largest |got - want| / |want| over the entries (0 where both are 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got != 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ pk_motion_stats
@pytest.mark.parametrize("T", [1, 2, 3, 255, 256, 257, 600])
def test_motion_stats_equal_the_restatement(T):
    from infantposeestimation_gaussianbias_amd import hipops
    tol, worst, kinds = (T + 16) * 2.0 ** -52, 0.0, set()
    for S in (1, 3):
        for K in (1, 13, 17):
            for with_conf in (False, True):
                seed = T + K                                      # moves the kinds of joints around, so that K = 1 meets each of them
                c, conf = mnp.motion_case(S, T, K, with_conf, seed)
                kinds |= {mnp.joint_kind(s, k, K, seed) for s in range(S) for k in range(K)}
                want = mnp.motion_stats(c, conf, 0.3)
                dc, dconf = G(c), None if conf is None else G(conf)
                got_t = hipops.motion_stats(dc, dconf, 0.3)
                again = hipops.motion_stats(dc, dconf, 0.3)
                assert torch.equal(got_t.view(torch.int64), again.view(torch.int64)), "two launches differ in their bits"
                got = got_t.cpu().numpy()
                assert got.shape == (S, K, 11) and got.dtype == np.float64
                for col in EXACT_COLS:
                    assert np.array_equal(got[..., col], want[..., col]), (S, K, with_conf, col)
                err = max(_rel(got[..., col], want[..., col]) for col in SUM_COLS)
                worst = max(worst, err)
                assert err <= tol, (S, K, with_conf, err, tol)
    assert kinds == set(mnp.KINDS)
    print(f"T={T}: largest relative error of the float64 columns {worst:.3e} (bound {tol:.3e})")


def test_motion_stats_validity_by_hand():
    """Five frames, frame 2 below the confidence threshold and frame 1 exactly at it: 4 valid frames, steps 0->1 and 3->4, no triple."""
    from infantposeestimation_gaussianbias_amd import hipops
    pts = np.array([[0, 0], [3, 4], [100, 100], [6, 8], [6, 8]], np.float32)[None, :, None, :]
    conf = np.array([0.9, np.float32(0.3), 0.1, 0.9, 0.9], np.float32)[None, :, None]
    assert hipops.motion_stats(G(pts), G(conf), 0.3).cpu().numpy()[0, 0].tolist() == [4, 0, 6, 0, 8, 10, 5, 2, 5, 0, 0]
    z = hipops.motion_stats(torch.zeros(2, 0, 3, 2, device=DEV))
    assert z.shape == (2, 3, 11) and not z.any()


# ------------------------------------------------------------------------------------------------ pk_position_histogram
HIST_CASES = [  # S, T, K, W, H, nbx, nby
    (1, 1, 1, 7, 5, 1, 1), (1, 257, 3, 30, 20, 3, 2), (3, 1000, 17, 640, 480, 64, 48), (1, 1000, 2, 1280, 1280, 128, 128),
    (2, 257, 13, 333, 217, 33, 21), (1, 1000, 1, 30, 20, 3, 2), (1, 1, 17, 640, 480, 64, 48)]


@pytest.mark.parametrize("S,T,K,W,H,nbx,nby", HIST_CASES)
@pytest.mark.parametrize("with_conf", [False, True])
def test_position_histogram_equals_histogram2d(S, T, K, W, H, nbx, nby, with_conf):
    from infantposeestimation_gaussianbias_amd import hipops
    c, conf, ex, ey = mnp.histogram_case(S, T, K, W, H, nbx, nby, with_conf)
    want = mnp.histogram2d(c, ex, ey, conf, 0.5)
    dc, dconf = G(c), None if conf is None else G(conf)
    got_t = hipops.position_histogram(dc, ex, ey, dconf, 0.5)
    assert got_t.dtype == torch.int32 and tuple(got_t.shape) == (S, K, nby, nbx)
    got = got_t.cpu().numpy()
    assert np.array_equal(got, want)
    assert torch.equal(got_t, hipops.position_histogram(dc, G(ex, torch.float64), G(ey, torch.float64), dconf, 0.5))
    n_valid = int(mnp.valid_frames(c, conf, 0.5).sum())
    print(f"{S}x{T}x{K} in {nbx}x{nby} bins: {int(got.sum())} of {n_valid} valid frames counted, all bins equal to np.histogram2d")
    assert got.sum() <= n_valid and (T < 200 or 0 < got.sum() < n_valid)     # the larger cases hold valid points outside the range


def test_position_histogram_refuses_more_bins_than_fit():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    c = torch.zeros(1, 4, 1, 2, device=DEV)
    with pytest.raises(PoseKernelError, match=r"code -2.*129 x 128 bins.*larger bins"):
        hipops.position_histogram(c, np.linspace(0, 1290, 130), np.linspace(0, 1280, 129))
    z = hipops.position_histogram(torch.zeros(2, 0, 3, 2, device=DEV), np.linspace(0, 10, 5), np.linspace(0, 10, 3))
    assert tuple(z.shape) == (2, 3, 2, 4) and not z.any()


# ------------------------------------------------------------------------------------------------ pk_pck
def _pck_device(case, parts=1):
    from infantposeestimation_gaussianbias_amd import hipops
    pred, gt, vis, norm, thr = case
    buf = hipops.pck_buffers(pred.shape[1], len(thr), DEV)
    dthr = G(thr)
    for idx in np.array_split(np.arange(len(pred)), parts):
        hipops.pck_accumulate(G(pred[idx]), G(gt[idx]), G(vis[idx]), G(norm[idx]), dthr, *buf)
    return buf


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_pck_counts_equal_the_restatement(N):
    worst, tol = 0.0, (N + 16) * 2.0 ** -52
    for K in (1, 17):
        for n_thr in (1, 6, 16):
            case = mnp.pck_case(N, K, n_thr)
            correct, valid, err = mnp.pck(*case)
            assert correct[0, 0] == mnp.pck(*(a[2:] for a in case[:4]), case[4])[0][0, 0] + 1, "the tie on the circle is a hit, the ulp outside a miss"
            buf = _pck_device(case)
            again = _pck_device(case)
            assert all(torch.equal(a, b) for a, b in zip(buf[:2], again[:2])) and torch.equal(buf[2].view(torch.int64), again[2].view(torch.int64))
            got_c, got_v, got_e = (b.cpu().numpy() for b in buf)
            assert got_c.dtype == np.int64 and got_e.dtype == np.float64
            assert np.array_equal(got_c, correct) and np.array_equal(got_v, valid), (K, n_thr)
            e = _rel(got_e, err)
            worst = max(worst, e)
            assert e <= tol, (K, n_thr, e, tol)
            if N > 1:
                # two updates over a split batch: the same counts; the error sum adds the halves' sums, each within its own bound
                split = _pck_device(case, parts=2)
                assert torch.equal(split[0], buf[0]) and torch.equal(split[1], buf[1])
                assert _rel(split[2].cpu().numpy(), err) <= tol
    print(f"N={N}: counts equal; largest relative error of err_sum {worst:.3e} (bound {tol:.3e})")


def test_pck_empty_batch_launches_nothing():
    from infantposeestimation_gaussianbias_amd import hipops
    buf = hipops.pck_buffers(3, 2, DEV)
    z = torch.zeros
    hipops.pck_accumulate(z(0, 3, 2, device=DEV), z(0, 3, 2, device=DEV), z(0, 3, device=DEV), z(0, device=DEV), z(2, device=DEV), *buf)
    assert not any(b.any() for b in buf)


# ------------------------------------------------------------------------------------------------ public functions
def test_public_functions_keep_the_kind_of_their_input():
    from infantposeestimation_gaussianbias_amd import utils
    c, conf = mnp.motion_case(1, 257, 13, True, 3)
    seq, cf = c[0], conf[0]
    want = mnp.motion_stats(c, conf, 0.3)[0]
    amp = utils.calculate_movement_amplitude(seq, cf)
    assert isinstance(amp, np.ndarray) and amp.shape == (13,) and _rel(amp, want[:, 5]) <= 32 * 2.0 ** -52
    amp_t = utils.calculate_movement_amplitude(G(seq), G(cf[..., None]))
    assert torch.is_tensor(amp_t) and amp_t.is_cuda and np.array_equal(amp_t.cpu().numpy(), amp)
    assert np.array_equal(utils.calculate_movement_amplitude(seq, cf[..., None]), amp)
    tc = utils.calculate_temporal_consistency(seq, cf)
    assert isinstance(tc, float) and abs(tc - want[:, 9].sum() / want[:, 10].sum()) <= (257 + 16) * 2.0 ** -52 * tc
    assert utils.calculate_temporal_consistency(seq[:2]) == 0.0
    no_conf = utils.calculate_movement_amplitude(seq)
    assert _rel(no_conf, mnp.motion_stats(c)[0][:, 5]) <= 32 * 2.0 ** -52 and not np.array_equal(no_conf, amp)
    hm = utils.movement_heatmap(seq, (480, 640), confidence=cf)
    assert isinstance(hm, np.ndarray) and hm.dtype == np.int32 and hm.shape == (13, 48, 64)
    assert np.array_equal(hm, mnp.histogram2d(c, np.linspace(0, 640, 65), np.linspace(0, 480, 49), conf, 0.3)[0])
    hm_t = utils.movement_heatmap(G(seq), (480, 640), confidence=G(cf))
    assert torch.is_tensor(hm_t) and hm_t.is_cuda and np.array_equal(hm_t.cpu().numpy(), hm)


def test_calculate_pck_and_the_accumulator():
    from infantposeestimation_gaussianbias_amd import utils
    pred, gt, vis, norm, thr = mnp.pck_case(257, 17, 6)
    correct, valid, err = mnp.pck(pred, gt, vis, norm, thr)
    res = utils.calculate_pck(pred, gt, vis, norm, thresholds=[float(t) for t in thr])
    seen = valid > 0
    assert set(res) == {f"PCK@{float(t):g}" for t in thr} | {"per_joint", "mean_error"}
    for j, t in enumerate(thr):
        assert res[f"PCK@{float(t):g}"] == float((correct[j, seen] / valid[seen]).mean())
    assert np.array_equal(res["per_joint"][:, seen], correct[:, seen] / valid[seen])
    assert abs(res["mean_error"] - err.sum() / valid.sum()) <= (257 * 17 + 16) * 2.0 ** -52 * res["mean_error"]
    acc = utils.PCKAccumulator(17, [float(t) for t in thr])
    assert acc.compute()["PCK@0.5"] == 0.0
    acc.update(G(pred[:100]), G(gt[:100]), G(vis[:100]), G(norm[:100]))
    acc.update(pred[100:], gt[100:], vis[100:], norm[100:])
    got = acc.counts()
    assert np.array_equal(got[0], correct) and np.array_equal(got[1], valid)
    json.dumps({k: v for k, v in acc.compute().items() if k != "per_joint"})


def test_movement_report_on_the_quick_start_wrists():
    from infantposeestimation_gaussianbias_amd import utils
    seq = mnp.quick_start_wrists()
    st = mnp.motion_stats(seq[None])[0]
    rep = utils.movement_report(seq, flip_pairs=[(0, 1)])
    assert json.loads(json.dumps(rep)) == rep
    assert [j["flag"] for j in rep["joints"]] == [mnp.flag(st[0, 5]), mnp.flag(st[1, 5])] == [None, None]
    pair = rep["pairs"][0]
    assert abs(pair["ratio"] - mnp.asymmetry_ratio(st[0, 5], st[1, 5])) <= 1e-12 and pair["ratio"] < 0.2 and pair["asymmetric"] is False
    assert abs(rep["temporal_consistency"] - st[:, 9].sum() / st[:, 10].sum()) <= (300 + 16) * 2.0 ** -52 * rep["temporal_consistency"]
    for k, j in enumerate(rep["joints"]):
        assert _rel([j["amplitude"], j["path_length"], j["mean_speed"], j["max_speed"]], [st[k, 5], st[k, 6], st[k, 6] / st[k, 7], st[k, 8]]) <= 1e-12
        assert j["valid_fraction"] == 1.0
    fast = utils.movement_report(G(seq), flip_pairs=[(0, 1)], fps=30.0)
    for a, b in zip(rep["joints"], fast["joints"]):
        assert b["mean_speed"] == a["mean_speed"] * 30.0 and b["max_speed"] == a["max_speed"] * 30.0 and b["amplitude"] == a["amplitude"]
    assert rep["speed_unit"] == "px/frame" and fast["speed_unit"] == "px/s"
    # the thresholds: 60 px of amplitude is low under 100 and high over 50; a still joint against a moving one is asymmetric
    tight = utils.movement_report(seq, flip_pairs=[(0, 1)], min_movement=100.0)
    loose = utils.movement_report(seq, flip_pairs=[(0, 1)], max_movement=50.0)
    assert [j["flag"] for j in tight["joints"]] == ["low", "low"] and [j["flag"] for j in loose["joints"]] == ["high", "high"]
    still = seq.copy()
    still[:, 1] = still[0, 1]
    lop = utils.movement_report(still, flip_pairs=[(0, 1)])
    assert lop["pairs"][0] == {"left": 0, "right": 1, "ratio": 1.0, "asymmetric": True} and lop["joints"][1]["flag"] == "low"
    still[:, 0] = still[0, 0]
    assert utils.movement_report(still, flip_pairs=[(0, 1)])["pairs"][0]["ratio"] == 0.0


def test_movement_heatmap_overlays_where_the_counts_are():
    from infantposeestimation_gaussianbias_amd import utils
    seq = mnp.quick_start_wrists()                                # x in 170..430, y in 270..330 of a 480 x 640 frame
    counts = utils.movement_heatmap(G(seq), (480, 640), bin_size=10)
    assert counts.shape == (2, 48, 64) and int(counts.sum()) == 2 * len(seq)
    frame = np.full((480, 640, 3), 90, np.uint8)
    out = utils.draw_heatmaps(frame, counts.float())
    assert out.shape == frame.shape and out.dtype == np.uint8
    # draw_heatmaps blends EVERY pixel with the colour of its index, index 0 (the ramp's dark blue) included: "unchanged" is the picture of
    # an all-zero map, one flat tint
    flat = utils.draw_heatmaps(frame, torch.zeros_like(counts, dtype=torch.float32))
    assert (flat == flat[0, 0]).all() and (flat != frame).any()
    changed = (out != flat).any(-1)
    # the overlay stretches the (48, 64) plane over the frame bilinearly: a pixel can only change where one of the bins around it is
    # positive, i.e. inside the positive bins grown by one bin; and it does change at the centre of every positive bin
    pos = counts.sum(0).cpu().numpy() > 0
    grown = np.zeros_like(pos)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            grown[max(dy, 0):48 + min(dy, 0), max(dx, 0):64 + min(dx, 0)] |= pos[max(-dy, 0):48 + min(-dy, 0), max(-dx, 0):64 + min(-dx, 0)]
    reach = np.kron(grown, np.ones((10, 10), bool))
    assert changed.any() and not (changed & ~reach).any()
    ys, xs = np.nonzero(pos)
    assert changed[ys * 10 + 5, xs * 10 + 5].all()


# ------------------------------------------------------------------------------------------------ validate.py
@functools.lru_cache(maxsize=None)
def _model(name="hrnet_w18"):
    import os
    from conftest import GOLDEN
    from recipe import synth_state_dict
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        keys = json.load(f)
    m = PoseEstimator("hrnet_w18", 17, False, "heatmap", True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(keys["hrnet_w18_heatmap"], 41).items()}, strict=True)
    return m.to(DEV).eval()


def test_validate_reports_pck_next_to_the_unchanged_metrics(monkeypatch):
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import SyntheticLoader
    from infantposeestimation_gaussianbias_amd.utils import metrics as metrics_mod
    cfg = get_config("hrnet_w18")
    cfg.train.batch_size = 4
    log, dev = logging.getLogger("test"), torch.device(DEV)
    seen, made = [], []

    class Recording(metrics_mod.PCKAccumulator):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def update(self, pred, gt, visible, normalizer):
            seen.append(tuple(t.detach().cpu().numpy().copy() for t in (pred, gt, visible, normalizer)))
            return super().update(pred, gt, visible, normalizer)

    plain, _ = V.validate(_model(), SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False)
    monkeypatch.setattr(metrics_mod, "PCKAccumulator", Recording)
    with_pck, _ = V.validate(_model(), SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False, pck_thresholds=(0.2, 0.5))
    assert set(with_pck) == set(plain) | {"PCK@0.2", "PCK@0.5", "PCK_mean_error"}
    assert 0.0 <= with_pck["PCK@0.2"] <= with_pck["PCK@0.5"] <= 1.0 and with_pck["PCK_mean_error"] > 0
    # the same image-space tensors through the restatement: equal counts; the normaliser is the longer side of the synthetic box
    assert len(seen) == 2 and len(made) == 1 and all(s[0].shape == (4, 17, 2) and np.all(s[3] == 128.0) for s in seen)
    correct, valid, err = mnp.pck(*(np.concatenate([s[i] for s in seen]) for i in range(4)), [0.2, 0.5])
    got = made[0].counts()
    assert np.array_equal(got[0], correct) and np.array_equal(got[1], valid) and _rel(got[2], err) <= (8 + 16) * 2.0 ** -52
    ok = valid > 0
    assert with_pck["PCK@0.5"] == float((correct[1, ok] / valid[ok]).mean())
    monkeypatch.undo()
    again, _ = V.validate(_model(), SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False)
    assert set(again) == set(plain) and not any(k.startswith("PCK") for k in again)


# ------------------------------------------------------------------------------------------------ inference.py
def test_predict_sequence_is_predict_batch_batch_by_batch():
    import inference
    from infantposeestimation_gaussianbias_amd import utils
    torch.manual_seed(11)
    pose = inference.PoseInference(config="hrnet_w18", flip_test=False)
    frames = [f for f in np.random.default_rng(12).integers(0, 256, (5, 120, 160, 3)).astype(np.uint8)]
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    kp, sc = pose.predict_sequence(frames, bbox, batch_size=2)
    assert kp.is_cuda and sc.is_cuda and tuple(kp.shape) == (5, 17, 2) and tuple(sc.shape) == (5, 17)
    parts = [pose.predict_batch(frames[i:i + 2], [bbox] * len(frames[i:i + 2])) for i in (0, 2, 4)]
    want_kp = np.concatenate([np.stack([r[0] for r in p]) for p in parts])
    want_sc = np.concatenate([np.stack([r[1] for r in p]) for p in parts])
    assert np.array_equal(kp.cpu().numpy().view(np.uint32), want_kp.astype(np.float32).view(np.uint32))
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), want_sc.astype(np.float32).view(np.uint32))
    assert want_kp.dtype == np.float32 and want_sc.dtype == np.float32
    pairs = pose.cfg.data.flip_pairs
    assert utils.movement_report(kp, sc, flip_pairs=pairs) == utils.movement_report(want_kp, want_sc, flip_pairs=pairs)
    whole, _ = pose.predict_sequence(frames[:1], None, batch_size=16)
    assert np.array_equal(whole.cpu().numpy()[0], pose.predict(frames[0])[0])
    report, kp_s, _ = inference.sequence_report(pose, frames, bbox, smooth=3, fps=25.0)
    assert report["smoothing"] == [3, "gaussian"] and report["num_frames"] == 5 and json.loads(json.dumps(report)) == report
    assert torch.equal(kp_s, utils.postprocess.temporal_smoothing(kp, 3, "gaussian"))
