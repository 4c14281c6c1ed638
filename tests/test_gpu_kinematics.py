"""Limb kinematics on the device: the five entries of csrc/pk_kinematics.hip against their numpy restatement (tests/kinematics_np.py) at the
sizes where each kernel changes behaviour -- the 256 elements a thread strides by, the sides of an entropy tile, lags beyond the sequence,
counts beyond 2^31, tile numbers beyond 65 535 -- their bit-for-bit promises, and the public functions.

Tolerances (derived, not measured; every test prints what it saw).
  angles   the NaN pattern is equal; |d theta| <= 16 2^-52 pi: both sides form cr and dt with identical single-rounded operations on bit-equal
           inputs, so only atan2 differs (two libraries, a few ulps each of a result of at most pi).
  speeds   relative 4 2^-52: sqrt is correctly rounded on both sides and its argument is bit-equal.
  stats    n, min, max, the step count and the largest step are equal.  mean within (n + 16) 2^-52 sum|x| / n (n additions at 2^-53 of partial
           sums bounded by sum|x|, in another order); sd and the step sum relative (n + 16) 2^-52 against the restatement evaluated WITH the
           device's stored mean bits (sums of non-negative terms).
  xcorr    counts equal; |dr| <= (n + 16) 2^-50 absolute: the n products and additions are at 2^-53 each, and by Cauchy-Schwarz
           sum |dx||dy| <= sqrt(sxx syy), so the bound is on r itself.  tests/test_kinematics_host.py measures the two summation orders against
           each other.  The summary equals the restatement's summary of the DEVICE's r bits exactly.
  entropy  exact integer equality, given the device's own tol bits.
Observed on one MI355X, as shares of these bounds: angles 4.0e-2, speeds equal, mean 1.5e-2, sd 9.1e-3, step sum 1.2e-2, xcorr 2.1e-2; the
two closed-form entropy cases took 1.5 ms (T = 70 003) and 5.3 ms (T = 140 003), so neither T was lowered."""
import json
import time

import numpy as np
import pytest
import torch

import kinematics_np as knp

pytestmark = pytest.mark.gpu
DEV = "cuda"


def G(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy, in the array's own type


def bits(t):
    return t.contiguous().view(torch.int64)


def _tile():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib.CONSTANTS["PK_KIN_ENTROPY_TILE"]


# ------------------------------------------------------------------------------------------------ angles and speeds
def test_angles_and_speeds_equal_the_restatement():
    from infantposeestimation_gaussianbias_amd import hipops
    S, T, K = 3, 67, 17
    c, conf = knp.kinematics_case(S, T, K)
    triples = list(knp.COCO_ANGLES.values()) + [(5, 7, 9)]
    # planted on the left elbow (5, 7, 9) of sequence 0: collinear both ways, a wrist on the elbow, a shoulder below the threshold
    c[0, 3:7, 7], conf[0, 3:7, 5:10] = (100.0, 200.0), 0.9
    c[0, 3, 5], c[0, 3, 9] = (103.0, 204.0), (106.0, 208.0)
    c[0, 4, 5], c[0, 4, 9] = (103.0, 204.0), (94.0, 192.0)
    c[0, 5, 5], c[0, 5, 9] = (103.0, 204.0), (100.0, 200.0)
    c[0, 6, 5], c[0, 6, 9], conf[0, 6, 5] = (103.0, 204.0), (94.0, 192.0), 0.29
    want = knp.joint_angles(c, conf, 0.3, triples)
    got_t = hipops.joint_angles(G(c), G(conf), 0.3, triples)
    got = got_t.cpu().numpy()
    assert got.shape == (S, T, 9) and got.dtype == np.float64
    assert torch.equal(bits(got_t), bits(hipops.joint_angles(G(c), G(conf), 0.3, triples)))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and 0.1 < np.isnan(want).mean() < 0.9
    err = float(np.nanmax(np.abs(got - want)))
    print(f"angles: largest difference {err / (16 * 2.0 ** -52 * np.pi):.3e} of the bound")
    assert err <= 16 * 2.0 ** -52 * np.pi and np.nanmin(got) >= 0 and np.nanmax(got) <= np.pi
    assert got[0, 3, 0] == 0.0 and got[0, 4, 0] == np.pi and np.isnan(got[0, 5, 0]) and np.isnan(got[0, 6, 0])
    assert np.array_equal(got[..., 0], got[..., 8], equal_nan=True)
    open_ = hipops.joint_angles(G(c), None, 0.3, triples).cpu().numpy()           # without confidences the shoulder counts
    assert open_[0, 6, 0] == np.pi and np.array_equal(np.isnan(open_), np.isnan(knp.joint_angles(c, None, 0.3, triples)))

    sw = knp.joint_speeds(c, conf, 0.3)
    sg = hipops.joint_speeds(G(c), G(conf), 0.3).cpu().numpy()
    assert sg.shape == (S, T, K) and np.array_equal(np.isnan(sg), np.isnan(sw)) and np.isnan(sg[:, -1]).all()
    live = ~np.isnan(sw)
    rel = float((np.abs(sg[live] - sw[live]) / np.maximum(sw[live], 1e-300)).max())
    print(f"speeds: largest relative difference {rel / (4 * 2.0 ** -52):.3e} of the bound")
    assert rel <= 4 * 2.0 ** -52 and live.sum() > S * T * K // 3
    empty = hipops.joint_angles(torch.zeros(0, 5, 17, 2, device=DEV), None, 0.3, triples)
    assert empty.shape == (0, 5, 9) and hipops.joint_speeds(torch.zeros(2, 0, 17, 2, device=DEV)).shape == (2, 0, 17)


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 600])
def test_series_stats_equal_the_restatement(T):
    """One below, at and above the 256 elements a thread strides by; T = 1: no step; series 1 is all NaN, series 2 has one valid element."""
    from infantposeestimation_gaussianbias_amd import hipops
    x = knp.series_case(3, T, 5, seed=T)
    got_t = hipops.series_stats(G(x))
    assert torch.equal(bits(got_t), bits(hipops.series_stats(G(x)))), "two launches differ in their bits"
    got = got_t.cpu().numpy()
    want = knp.series_stats(x)
    with_mean = knp.series_stats(x, mean=got[..., 3])
    n = want[..., 0]
    for col in (0, 1, 2, 6, 7):
        assert np.array_equal(got[..., col], want[..., col]), col
    assert not got[:, 1].any() and got[:, 2, 0].tolist() == [1.0] * 3 and got[:, 2, 1:5].tolist() == [[1.25, 1.25, 1.25, 0.0]] * 3
    sum_abs = np.abs(np.where(np.isfinite(x), x, 0.0)).sum(1)
    bound = (n + 16) * 2.0 ** -52 * sum_abs / np.maximum(n, 1)
    m_err = np.abs(got[..., 3] - want[..., 3])
    assert (m_err <= bound).all()
    shares = [float((m_err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0]
    for col in (4, 5):
        w = with_mean[..., col]
        rel = np.where(w != 0, np.abs(got[..., col] - w) / np.where(w != 0, np.abs(w), 1.0), np.where(got[..., col] != 0, np.inf, 0.0))
        shares.append(float((rel / ((n + 16) * 2.0 ** -52)).max()))
        assert (rel <= (n + 16) * 2.0 ** -52).all(), col
    print(f"T={T}: mean {shares[0]:.3e}, sd {shares[1]:.3e}, step sum {shares[2]:.3e} of their bounds")


# ------------------------------------------------------------------------------------------------ cross-correlation
def _xcorr_case(T):
    x = knp.series_case(2, T, 5, seed=3 * T, gap_share=0.15)
    x[:, :, 4] = 2.5                                              # a constant series
    if T > 40:
        x[0, 10:T - 10, 3] = np.nan                               # series 3 of sequence 0 keeps its ends only: most lags starve
    return x, [(0, 0), (0, 3), (3, 0), (4, 3)]


@pytest.mark.parametrize("T", [2, 64, 257, 513])
def test_xcorr_equals_the_restatement(T):
    from infantposeestimation_gaussianbias_amd import hipops
    x, pairs = _xcorr_case(T)
    dx = G(x)
    worst, starved = 0.0, 0
    for L in (0, 7, T - 1, T + 3):
        r_t, n_t, s_t = hipops.series_xcorr(dx, pairs, L, 3)
        r2, n2, s2 = hipops.series_xcorr(dx, pairs, L, 3)
        assert torch.equal(bits(r_t), bits(r2)) and torch.equal(n_t, n2) and torch.equal(bits(s_t), bits(s2)), "two launches differ in their bits"
        r, n, summ = r_t.cpu().numpy(), n_t.cpu().numpy(), s_t.cpu().numpy()
        want_r, want_n = knp.xcorr(x, pairs, L)
        assert r.shape == (2, 4, 2 * L + 1) and n.dtype == np.int32 and np.array_equal(n, want_n)
        share = np.abs(r - want_r) / ((n + 16) * 2.0 ** -50)
        worst, starved = max(worst, float(share.max())), starved + int((n < 3).sum())
        assert (share <= 1.0).all() and not r[n < 2].any() and not r[:, 3].any() and np.abs(r).max() <= 1 + 1e-12
        assert np.array_equal(summ, knp.xcorr_summary(r, n, 3)), "the summary is not that of the stored r"
        assert torch.equal(bits(r_t[:, 1]), bits(r_t[:, 2].flip(-1))) and torch.equal(n_t[:, 1], n_t[:, 2].flip(-1)), "(i, j) at l against (j, i) at -l"
        if L >= T:
            assert not n[..., :L - T + 1].any() and not n[..., L + T:].any() and n[0, 0, L] > 0
    print(f"T={T}: xcorr error {worst:.3e} of its bound, {starved} lags below min_count")
    assert starved > 0


def test_xcorr_bits_depend_neither_on_the_batch_nor_on_the_lags():
    from infantposeestimation_gaussianbias_amd import hipops
    x, pairs = _xcorr_case(257)
    dx = G(x)
    r, n, _ = hipops.series_xcorr(dx, pairs, 40)
    for p in range(4):                                            # one pair alone
        r1, n1, _ = hipops.series_xcorr(dx, pairs[p:p + 1], 40)
        assert torch.equal(bits(r1[:, 0]), bits(r[:, p])) and torch.equal(n1[:, 0], n[:, p]), f"pair {p} alone differs"
    for s in range(2):                                            # one sequence alone
        r1, _, _ = hipops.series_xcorr(dx[s:s + 1].contiguous(), pairs, 40)
        assert torch.equal(bits(r1[0]), bits(r[s])), f"sequence {s} alone differs"
    for L in (0, 7, 39):                                          # fewer lags
        r1, n1, _ = hipops.series_xcorr(dx, pairs, L)
        assert torch.equal(bits(r1), bits(r[..., 40 - L:41 + L])) and torch.equal(n1, n[..., 40 - L:41 + L]), f"max_lag {L} differs"
    two = hipops.series_xcorr(dx[..., [0, 3]].contiguous(), [(0, 1)], 40)[0]       # the same two series in a narrower batch
    assert torch.equal(bits(two[:, 0]), bits(r[:, 1]))


# ------------------------------------------------------------------------------------------------ sample entropy
def _entropy_case(n, m, B0):
    """(3, n + m, 5): noise; all NaN; a 0.25 grid (exact ties at tol = 0.5); noise with NaN at B0 - 1, B0 and B0 + m - 1, so that the
    templates that straddle the first tile edge are the invalid ones; a smooth series."""
    T = n + m
    g = np.random.default_rng(100 * n + m)
    x = g.standard_normal((3, T, 5))
    x[:, :, 1] = np.nan
    x[:, :, 2] = g.integers(-4, 5, (3, T)) * 0.25
    for t in (B0 - 1, B0, B0 + m - 1):
        if t < T:
            x[:, t, 3] = np.nan
    x[:, :, 4] = np.sin(np.arange(T) / 5.0)[None] + 0.05 * g.standard_normal((3, T))
    return x


@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("n_tiles", ["0", "1", "2", "B0-1", "B0", "B0+1", "2*B0+1", "3*B0+5"])
def test_entropy_counts_equal_the_restatement(n_tiles, m):
    from infantposeestimation_gaussianbias_amd import hipops
    B0 = _tile()
    n = min(eval(n_tiles, {"B0": B0}), 1100)
    x = _entropy_case(n, m, B0)
    dx = G(x)
    tol = hipops.series_stats(dx)[..., 4] * 0.2
    tol[:, 2] = 0.5
    tol[2, 0], tol[2, 3], tol[1, 4] = -1.0, float("nan"), float("inf")
    tiles = hipops.sample_entropy_tiles(n + m, m)
    rows = 15 * tiles
    ws = torch.full((rows + 7, 2), -7, dtype=torch.int64, device=DEV)
    got = hipops.sample_entropy_counts(dx, tol, m, workspace=ws)
    assert got.shape == (3, 5, 3) and got.dtype == torch.int64
    assert torch.equal(got, hipops.sample_entropy_counts(dx, tol, m))
    want = knp.sample_entropy_counts(x, tol.cpu().numpy(), m)
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy() - want)
    ws = ws.cpu().numpy()
    assert (ws[:rows] >= 0).all() and (ws[rows:] == -7).all(), "the workspace query is not the number of rows written"
    assert not want[:, 1].any() and not want[2, 0, 1:].any() and not want[2, 3, 1:].any() and not want[1, 4, 1:].any()
    assert want[0, 0, 0] == n
    if n >= B0 - 1:
        assert want[0, 2, 2] > 0 and want[0, 4, 1] > 0
    if n > B0 + m:
        assert want[0, 3, 0] < n - m - 1                          # the gaps took more than m + 1 templates


def _constant_series_counts(T, limit_s):
    """B = A = n (n - 1) / 2 of a constant series, without an all-pairs array on the host."""
    from infantposeestimation_gaussianbias_amd import hipops
    x = torch.full((1, T, 1), 1.5, dtype=torch.float64, device=DEV)
    tol = torch.zeros(1, 1, dtype=torch.float64, device=DEV)
    hipops.sample_entropy_counts(x[:, :600].contiguous(), tol, 2)                 # the code object is loaded
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = hipops.sample_entropy_counts(x, tol, 2).cpu().numpy()[0, 0]
    took = time.perf_counter() - t0
    n = T - 2
    print(f"T={T}: {n * (n - 1) // 2} pairs, {hipops.sample_entropy_tiles(T, 2)} tiles, {took * 1e3:.1f} ms")
    assert got.tolist() == [n, n * (n - 1) // 2, n * (n - 1) // 2]
    assert took <= limit_s
    return n * (n - 1) // 2


def test_entropy_counts_pass_two_to_the_31():
    assert _constant_series_counts(70003, 5.0) > 1 << 31


def test_entropy_tile_numbers_pass_65535():
    from infantposeestimation_gaussianbias_amd import hipops
    assert hipops.sample_entropy_tiles(140003, 2) > 65535
    _constant_series_counts(140003, 5.0)


# ------------------------------------------------------------------------------------------------ public functions
def test_kinematics_report_finds_the_planted_elbows():
    """Both elbows flex sinusoidally between 40 and 150 degrees, the left one 6 frames ahead; the left ankle is driven by noise."""
    from infantposeestimation_gaussianbias_amd import hipops, utils
    from infantposeestimation_gaussianbias_amd.utils import metrics
    seq = knp.elbow_trajectory(300, lag=6, lo_deg=40.0, hi_deg=150.0)
    pairs = [(5, 6), (9, 10)]
    rep = utils.kinematics_report(seq, flip_pairs=pairs, fps=30.0)
    assert json.loads(json.dumps(rep)) == rep and rep["max_lag"] == 30 and rep["angular_speed_unit"] == "deg/s" and rep["num_frames"] == 300
    by_name = {a["name"]: a for a in rep["angles"]}
    assert list(by_name) == list(knp.COCO_ANGLES) and by_name["left_elbow"]["joints"] == [5, 7, 9]
    assert set(rep["angles"][0]) == {"name", "joints", "valid_fraction", "min_deg", "max_deg", "range_deg", "mean_deg", "sd_deg", "angular_path_deg",
                                     "mean_angular_speed", "max_angular_speed", "sample_entropy"}
    for side in ("left_elbow", "right_elbow"):
        a = by_name[side]
        assert abs(a["range_deg"] - 110.0) <= 0.5 and abs(a["min_deg"] - 40.0) <= 0.5 and abs(a["max_deg"] - 150.0) <= 0.5, a
        assert a["valid_fraction"] == 1.0 and abs(a["mean_angular_speed"] - a["angular_path_deg"] / 299 * 30.0) <= 1e-9
    coord = {(c["kind"], c["left"]): c for c in rep["coordination"]}
    assert len(coord) == 4 + 2 and set(rep["coordination"][0]) == {"kind", "left", "right", "r0", "peak_r", "peak_lag", "peak_lag_s", "pairs_used"}
    elbows = coord[("angle", "left_elbow")]
    assert elbows["peak_lag"] == 6 and elbows["peak_r"] > 0.99 and elbows["peak_lag_s"] == 0.2 and elbows["pairs_used"] == 294
    assert elbows["r0"] < elbows["peak_r"] and coord[("joint_speed", 9)]["peak_lag"] == 6
    assert by_name["left_elbow"]["sample_entropy"] < by_name["left_knee"]["sample_entropy"]
    assert len(rep["joints"]) == 17 and rep["joints"][9]["speed_entropy"] < rep["joints"][15]["speed_entropy"]
    # the kind of the input: numpy in -> numpy out, device in -> device out, and the same report either way
    assert utils.kinematics_report(G(seq), flip_pairs=pairs, fps=30.0) == rep
    th = utils.joint_angle_series(seq)
    th_dev = utils.joint_angle_series(G(seq))
    assert isinstance(th, np.ndarray) and th.shape == (300, 8) and torch.is_tensor(th_dev) and th_dev.is_cuda
    assert np.array_equal(th_dev.cpu().numpy(), th) and abs(np.degrees(th[12, 0]) - 150.0) <= 0.01
    co = utils.limb_coordination(th[:, 0], th[:, 1], 30, fps=30.0)
    assert isinstance(co["r"], np.ndarray) and co["r"].shape == (61,) and co["lags"][0] == -30 and co["pairs"][30] == 300
    assert {k: co[k] for k in ("r0", "peak_r", "peak_lag", "peak_lag_s", "pairs_used")} == {k: elbows[k] for k in elbows if k not in ("kind", "left", "right")}
    co_dev = utils.limb_coordination(th_dev[:, 0], th_dev[:, 1], 30)
    assert torch.is_tensor(co_dev["r"]) and co_dev["r"].is_cuda and np.array_equal(co_dev["r"].cpu().numpy(), co["r"]) and co_dev["peak_lag_s"] is None
    assert utils.sample_entropy(th[:, 0]) == by_name["left_elbow"]["sample_entropy"]
    assert utils.sample_entropy(th_dev[:, [0, 4]]) == [by_name["left_elbow"]["sample_entropy"], by_name["left_hip"]["sample_entropy"]]
    # movement_report: unchanged without `kinematics`, the same block with it
    plain = utils.movement_report(seq, flip_pairs=pairs, fps=30.0)
    stats = hipops.motion_stats(G(seq)[None], None, 0.3)[0].cpu().numpy()
    assert plain == metrics._report_from_stats(stats, 300, pairs, 5.0, 200.0, 0.2, 30.0) and "kinematics" not in plain
    both = utils.movement_report(seq, flip_pairs=pairs, fps=30.0, kinematics={})
    assert both["kinematics"] == rep and {k: v for k, v in both.items() if k != "kinematics"} == plain
    short = utils.movement_report(seq, flip_pairs=pairs, kinematics={"max_lag": 4, "entropy": (1, 0.3)})["kinematics"]
    assert short == utils.kinematics_report(seq, flip_pairs=pairs, max_lag=4, entropy=(1, 0.3)) and short["max_lag"] == 4
    assert short["coordination"][0]["peak_lag"] == 4 and short["entropy"] == {"m": 1, "r": 0.3} and short["angular_speed_unit"] == "deg/frame"


def test_sequence_report_adds_the_kinematics_block():
    import inference
    from infantposeestimation_gaussianbias_amd import utils
    torch.manual_seed(11)
    pose = inference.PoseInference(config="hrnet_w18", flip_test=False)
    frames = [f for f in np.random.default_rng(12).integers(0, 256, (4, 120, 160, 3)).astype(np.uint8)]
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    plain, kp, sc = inference.sequence_report(pose, frames, bbox, fps=24.0)
    assert "kinematics" not in plain
    report, kp2, sc2 = inference.sequence_report(pose, frames, bbox, fps=24.0, kinematics=True)
    assert torch.equal(kp, kp2) and torch.equal(sc, sc2) and json.loads(json.dumps(report)) == report
    assert {k: v for k, v in report.items() if k != "kinematics"} == plain
    block = report["kinematics"]
    want = utils.kinematics_report(kp, sc, flip_pairs=pose.cfg.data.flip_pairs, min_confidence=pose.cfg.min_keypoint_visibility, fps=24.0)
    assert block == want and block["max_lag"] == 2 and len(block["angles"]) == 8 and len(block["joints"]) == 17
    assert len(block["coordination"]) == 4 + len(pose.cfg.data.flip_pairs)
    pose.cfg.kinematics = {"max_lag": 1, "entropy": (1, 0.5)}    # the config's settings count, the caller's come first
    assert inference.sequence_report(pose, frames, bbox, kinematics=True)[0]["kinematics"]["entropy"] == {"m": 1, "r": 0.5}
    assert inference.sequence_report(pose, frames, bbox, kinematics={"max_lag": 0})[0]["kinematics"]["max_lag"] == 0
