"""Movement spectrum on the device: pk_motion_spectrum against its numpy restatement (tests/spectrum_np.py) at the sizes where the kernel
changes behaviour -- its 64-frame chunk per wave, its 256-frame LDS tile, its 64 bins per workgroup, a phase product beyond 2^32, joints
without power -- its bit-for-bit promises (repeatable, independent of the batch and of the band), and the public functions.

Tolerances (derived, not measured; every test prints what it saw).
  power    per bin |P_dev - P_np| <= (n + 16) 2^-50 scale, scale = 4 (sum_t |u_t.x| + |u_t.y|)^2 / W^2 of the joint: absolute and relative to
           the joint's scale, because bins that cancel have no meaningful relative error.  n products and additions at 2^-53 each, a few
           ulps for sin / cos, and the squares.
  summary  against the restatement's `summary` applied to the DEVICE's power bits: columns 0 (n) and 3 (peak bin) equal; column 1 (W)
           within (n + 16) 2^-52 of the restatement's W, relative like every sum of non-negative terms in tests/test_gpu_motion.py (n
           additions at 2^-53 of a partial sum that never exceeds W, and an ulp or two in each Hann weight; the rectangular W is exact);
           columns 2, 4, 5 within (F + 16) 2^-52 relative (F additions of non-negative terms in another order)."""
import json

import numpy as np
import pytest
import torch

import motion_np as mnp
import spectrum_np as snp

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK, TILE, BINS = 64, 256, 64                                   # SPEC_CHUNK, SPEC_TILE, SPEC_BINS of csrc/pk_spectrum.hip


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached cases are read-only


def bits(t):
    return t.contiguous().view(torch.int64)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got != 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def check(c, conf, N, j0, F, window, min_conf=0.3):
    """Launch twice, compare with the restatement under the tolerances of the module docstring.  -> (power, summary) tensors, the
    largest power error as a share of its bound."""
    from infantposeestimation_gaussianbias_amd import hipops
    dc, dconf = G(c), None if conf is None else G(conf)
    P_t, S_t = hipops.motion_spectrum(dc, dconf, min_conf, N, j0, F, window)
    P_2, S_2 = hipops.motion_spectrum(dc, dconf, min_conf, N, j0, F, window)
    assert torch.equal(bits(P_t), bits(P_2)) and torch.equal(bits(S_t), bits(S_2)), "two launches differ in their bits"
    P, summ = P_t.cpu().numpy(), S_t.cpu().numpy()
    S, T, K, _ = c.shape
    assert P.shape == (S, K, F) and summ.shape == (S, K, 6) and P.dtype == np.float64 and summ.dtype == np.float64
    want, n, W, scale = snp.power(c, conf, min_conf, N, j0, F, window)
    bound = (n + 16) * 2.0 ** -50 * scale
    err = np.abs(P - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.where(bound[..., None] > 0, err / bound[..., None], np.where(err > 0, np.inf, 0.0)).max())
    dead = scale == 0
    assert not P[dead].any(), "a joint with fewer than 2 valid frames, or none that moves, has no power"
    ws = snp.summary(P, summ[..., 0], summ[..., 1], j0)
    w_err = _rel(summ[..., 1], W) / ((n.max() + 16) * 2.0 ** -52)
    s_err = max(_rel(summ[..., col], ws[..., col]) for col in (2, 4, 5)) / ((F + 16) * 2.0 ** -52)
    print(f"S,T,K={S},{T},{K} N={N} j0={j0} F={F} window={window} conf={conf is not None}: power error {ratio:.3e} of its bound, "
          f"W {w_err:.3e} of its bound, summary sums {s_err:.3e} of theirs")
    assert ratio <= 1.0, ratio
    assert np.array_equal(summ[..., 0], n) and np.array_equal(summ[..., 3], ws[..., 3])
    assert np.all(np.abs(summ[..., 1] - W) <= (n + 16) * 2.0 ** -52 * W), w_err
    assert s_err <= 1.0 and np.array_equal(summ[..., 4], ws[..., 4])          # the peak's power is one of the stored values
    assert np.array_equal(summ[dead][:, 2:], np.tile([0.0, -1.0, 0.0, 0.0], (int(dead.sum()), 1)))
    return P_t, S_t, ratio


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("window", [0, 1])
def test_spectrum_equals_the_restatement(window, with_conf):
    """(S,T,K) = (2,257,3), zero-padded to N = 512, every bin 1 .. 256; plain, never-valid, alternating, gappy and non-finite joints and one
    with a single valid frame side by side."""
    c, conf = snp.spectrum_case(2, 257, 3, with_conf)
    n = mnp.valid_frames(c, conf, 0.3).sum(1)
    assert n[0, 1] == 0 and n[1, 2] == 1 and n[0, 0] == 257 and 100 < n[0, 2] < 200
    _, summ, _ = check(c, conf, 512, 1, 256, window)
    assert summ[0, 1].tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0] and summ[1, 2, 0] == 1 and summ[1, 2, 3] == -1


@pytest.mark.parametrize("T", [2, 3, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + CHUNK + 1])
def test_frame_tile_and_chunk_boundaries(T):
    """T one below, equal to and one above the 64 frames of a wave's chunk and the 256 frames of a tile; T = 2, 3: the shortest
    sequences with a spectrum; 577: a third tile that ends one frame into its second chunk."""
    c, conf = snp.spectrum_case(1, T, 3, True, seed=5 * T + 3)        # a gappy, a non-finite and a plain joint
    N = 2 * T + 6
    for window in (0, 1):
        check(c, conf, N, 1, min(N // 2, 70), window)


@pytest.mark.parametrize("F", [1, BINS - 1, BINS, BINS + 1])
def test_bins_per_workgroup_boundaries(F):
    c, conf = snp.spectrum_case(2, 130, 3, False, seed=F)
    check(c, conf, 300, 3, F, 1)


@pytest.mark.parametrize("N,j0", [(1 << 30, (1 << 29) - 300), (10 ** 9, 5 * 10 ** 8 - 300)])
def test_phase_product_beyond_32_bits(N, j0):
    """(j0 + j) t passes 2^32 (tests/test_spectrum_host.py shows that a 32-bit product gives other phases); the last bin is N / 2."""
    c, conf = snp.spectrum_case(1, 300, 2, False, seed=9)
    check(c, conf, N, j0, 301, 0)
    check(c, conf, N, j0, 301, 1)


def test_closed_forms_on_the_device():
    """A 30 px oscillation at bin 10 of 600 frames: sqrt(P) within 2^-14 px of 30 under both windows, Hann neighbours 15; a circle of radius
    25: 2 R^2; a constant joint and a single-frame joint: no power, peak -1."""
    from infantposeestimation_gaussianbias_amd import hipops
    T = 600
    c = np.zeros((1, T, 4, 2), np.float32)
    c[0, :, 0], c[0, :, 1], c[0, :, 2] = snp.oscillation(T, T, 10), snp.circle(T, T, 7, 25.0), (128.0, 64.0)
    c[0, :, 3] = np.nan
    c[0, 5, 3] = (3.0, 4.0)
    for window in (0, 1):
        P, summ = (t.cpu().numpy()[0] for t in hipops.motion_spectrum(G(c), None, 0.3, T, 1, T // 2, window))
        assert abs(np.sqrt(P[0, 9]) - 30.0) <= 2.0 ** -14 and abs(P[1, 6] - 1250.0) <= 100 * 2.0 ** -14
        assert summ[:, 3].tolist() == [10.0, 7.0, -1.0, -1.0] and not P[2:].any() and summ[:, 0].tolist() == [T, T, T, 1]
        if window:
            assert abs(np.sqrt(P[0, 8]) - 15.0) <= 2.0 ** -14 and abs(np.sqrt(P[0, 10]) - 15.0) <= 2.0 ** -14
        else:
            assert abs(summ[0, 5] - 10.0) <= 1e-6


# ------------------------------------------------------------------------------------------------ bit-for-bit promises
def test_bits_depend_neither_on_the_batch_nor_on_the_band():
    from infantposeestimation_gaussianbias_amd import hipops
    c, conf = snp.spectrum_case(3, 321, 5, True, seed=2)
    dc, dconf = G(c), G(conf)
    P, summ = hipops.motion_spectrum(dc, dconf, 0.3, 700, 2, 200, 1)
    for s in range(3):
        P1, s1 = hipops.motion_spectrum(dc[s:s + 1].contiguous(), dconf[s:s + 1].contiguous(), 0.3, 700, 2, 200, 1)
        assert torch.equal(bits(P1[0]), bits(P[s])) and torch.equal(bits(s1[0]), bits(summ[s])), f"sequence {s} alone differs from the batch"
    for k in (0, 4):                                              # one joint alone: K = 1
        P1, _ = hipops.motion_spectrum(dc[:, :, k:k + 1].contiguous(), dconf[:, :, k:k + 1].contiguous(), 0.3, 700, 2, 200, 1)
        assert torch.equal(bits(P1[:, 0]), bits(P[:, k])), f"joint {k} alone differs"
    for j0, F in ((2, 1), (70, 64), (101, 33), (201, 1), (130, 72)):          # other lanes, other workgroups, other neighbours
        Pb, sb = hipops.motion_spectrum(dc, dconf, 0.3, 700, j0, F, 1)
        assert torch.equal(bits(Pb), bits(P[..., j0 - 2:j0 - 2 + F])), f"band {j0}..{j0 + F - 1} alone differs from the wide launch"
        assert torch.equal(bits(sb[..., :2]), bits(summ[..., :2]))


# ------------------------------------------------------------------------------------------------ public functions
def test_movement_spectrum_keeps_the_kind_of_its_input():
    from infantposeestimation_gaussianbias_amd import utils
    c, conf = snp.spectrum_case(1, 257, 13, True, seed=3)
    seq, cf, fps = c[0].copy(), conf[0].copy(), 30.0             # the cached case is read-only
    out = utils.movement_spectrum(seq, fps, cf, f_min=0.5, f_max=6.0, n_fft=512)
    j0, F = snp.band_bins(fps, 512, 0.5, 6.0)
    want, n, W, scale = snp.power(c, conf, 0.3, 512, j0, F, 1)
    assert set(out) == {"frequencies", "power", "peak_frequency", "peak_amplitude", "band_power", "mean_frequency"}
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in out.values())
    assert np.array_equal(out["frequencies"], (j0 + np.arange(F)) / 512 * fps) and out["frequencies"][0] >= 0.5 and out["frequencies"][-1] <= 6.0
    assert out["power"].shape == (13, F) and np.all(np.abs(out["power"] - want[0]) <= ((n + 16) * 2.0 ** -50 * scale)[0][:, None])
    ws = snp.summary(out["power"], n[0], W[0], j0)
    live = ws[:, 3] >= 0
    assert (~live).any() and live.sum() > 8 and np.isnan(out["peak_frequency"][~live]).all()
    assert np.array_equal(out["peak_frequency"][live], ws[live, 3] / 512 * fps) and np.array_equal(out["peak_amplitude"], np.sqrt(ws[:, 4]))
    assert _rel(out["band_power"], ws[:, 2]) <= (F + 16) * 2.0 ** -52 and _rel(out["mean_frequency"], ws[:, 5] / 512 * fps) <= (F + 18) * 2.0 ** -52
    dev = utils.movement_spectrum(G(seq), fps, G(cf[..., None]), f_min=0.5, f_max=6.0, n_fft=512)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float64 for v in dev.values())
    for key, v in out.items():
        if key == "peak_amplitude":                               # a square root taken on the device, not on the host: an ulp
            assert _rel(dev[key].cpu().numpy(), v) <= 2.0 ** -52
        else:
            assert np.array_equal(dev[key].cpu().numpy(), v, equal_nan=True), key
    full = utils.movement_spectrum(seq, fps, window="rect")
    assert full["power"].shape == (13, 128) and full["frequencies"][-1] == 128 / 257 * fps


def test_movement_report_finds_a_planted_oscillation():
    """A 20 px oscillation at 1.5 Hz on the left joint and at 2.5 Hz on the right one, 30 fps, 10 s, on top of a slow drift."""
    from infantposeestimation_gaussianbias_amd import utils
    T, fps = 300, 30.0
    t = np.arange(T) / fps
    seq = np.zeros((T, 3, 2), np.float32)
    seq[:, 0, 0], seq[:, 0, 1] = 200 + 20 * np.sin(2 * np.pi * 1.5 * t), 300 + 0.02 * np.arange(T)
    seq[:, 1, 0], seq[:, 1, 1] = 400 + 20 * np.sin(2 * np.pi * 2.5 * t + 1.0), 300
    seq[:, 2] = (128.0, 64.0)
    plain = utils.movement_report(seq, flip_pairs=[(0, 1)], fps=fps)
    rep = utils.movement_report(seq, flip_pairs=[(0, 1)], fps=fps, spectrum=(0.5, 5.0))
    assert json.loads(json.dumps(rep)) == rep and rep["frequency_band"] == [0.5, 5.0]
    one_bin = fps / T
    assert abs(rep["joints"][0]["dominant_frequency"] - 1.5) <= one_bin and abs(rep["joints"][1]["dominant_frequency"] - 2.5) <= one_bin
    assert abs(rep["joints"][0]["peak_amplitude"] - 20.0) <= 0.5 and rep["joints"][0]["band_power"] >= rep["joints"][0]["peak_amplitude"] ** 2
    assert rep["joints"][2]["dominant_frequency"] is None and rep["joints"][2]["peak_amplitude"] == 0.0 and rep["joints"][2]["band_power"] == 0.0
    assert abs(rep["pairs"][0]["frequency_difference"] - 1.0) <= 2 * one_bin
    # the same numbers as movement_spectrum's, and without `spectrum` the report of before
    spec = utils.movement_spectrum(seq, fps, f_min=0.5, f_max=5.0)
    assert rep["joints"][0]["dominant_frequency"] == spec["peak_frequency"][0] and rep["joints"][1]["band_power"] == spec["band_power"][1]
    for j in rep["joints"]:
        for key in ("dominant_frequency", "peak_amplitude", "band_power"):
            del j[key]
    del rep["pairs"][0]["frequency_difference"], rep["frequency_band"]
    assert rep == plain
    assert utils.movement_report(G(seq), flip_pairs=[(0, 1)], fps=fps) == plain


def test_sequence_report_adds_the_spectrum_of_the_band():
    import inference
    from infantposeestimation_gaussianbias_amd import utils
    torch.manual_seed(11)
    pose = inference.PoseInference(config="hrnet_w18", flip_test=False)
    frames = [f for f in np.random.default_rng(12).integers(0, 256, (6, 120, 160, 3)).astype(np.uint8)]
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    plain, kp, sc = inference.sequence_report(pose, frames, bbox, fps=24.0)
    assert "frequency_band" not in plain and "dominant_frequency" not in plain["joints"][0]
    report, kp2, sc2 = inference.sequence_report(pose, frames, bbox, fps=24.0, freq_band=[3.0, 12.0])          # bins 1 .. 3 of 6 frames: 4, 8, 12 Hz
    assert torch.equal(kp, kp2) and torch.equal(sc, sc2) and json.loads(json.dumps(report)) == report
    pairs = pose.cfg.data.flip_pairs
    want = utils.movement_report(kp, sc, flip_pairs=pairs, min_confidence=pose.cfg.min_keypoint_visibility, fps=24.0, spectrum=(3.0, 12.0))
    assert {k: v for k, v in report.items() if k != "smoothing"} == want and report["frequency_band"] == [3.0, 12.0]
    assert all(j["dominant_frequency"] in (None, 4.0, 8.0, 12.0) for j in report["joints"]) and len(report["pairs"]) == len(pairs)
    pose.cfg.frequency_band = (3.0, 12.0)                         # the config's band counts when the frame rate is known
    assert inference.sequence_report(pose, frames, bbox, fps=24.0)[0] == report
    assert inference.sequence_report(pose, frames, bbox)[0]["fps"] is None
    with pytest.raises(ValueError, match="needs fps"):
        inference.sequence_report(pose, frames, bbox, freq_band=[3.0, 12.0])
