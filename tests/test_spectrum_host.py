"""Movement spectrum without a GPU: the numpy restatement (tests/spectrum_np.py) against np.fft.rfft and closed forms, the entry's
declaration and argument checks (which run before anything touches a device), the ValueErrors of the public functions, the legacy-yaml key
and the unchanged report.  The library function itself raises without a device, so nothing here calls it past its argument checks."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import motion_np as mnp
import spectrum_np as snp

F32 = np.float32


# ------------------------------------------------------------------------------------------------ restatement against np.fft.rfft
@pytest.mark.parametrize("window", [0, 1])
def test_restatement_equals_rfft_of_the_detrended_samples(window):
    """T = 257 frames zero-padded to N = 512, every bin from 1 to 256, gaps planted: NaN / inf coordinates and confidences below the
    threshold.  rfft sums u_t exp(-i ang), the restatement u_t (cos ang, sin ang): the same magnitudes.  The difference is scaled as
    the device tolerance is, by 4 (sum |u|)^2 / W^2; two float64 evaluations of the same sums agree to a few 1e-16 of that scale, and
    1e-13 is still three orders below the (n + 16) 2^-50 the device is given."""
    T, N, j0, F = 257, 512, 1, 256
    g = np.random.default_rng(5)
    c = (np.array([320.0, 240.0]) + np.cumsum(g.standard_normal((2, T, 3, 2)) * 3.0, axis=1)).astype(F32)
    conf = (0.5 + 0.5 * g.random((2, T, 3))).astype(F32)
    c[0, 17, 0, 0], c[0, 99, 0, 1], c[1, 200, 2, 0] = np.nan, np.inf, -np.inf
    conf[0, 40:60, 1], conf[1, 3, 0], conf[1, 128, 1] = 0.1, 0.29, F32(0.3)         # exactly at the threshold counts
    P, summ, scale = snp.spectrum(c, conf, 0.3, N, j0, F, window)
    n, W, u, live = snp.detrended(c, conf, 0.3, window)
    assert live.all() and n[0, 1] == T - 20 and n[0, 0] == T - 2 and n[1, 0] == T - 1 and n[1, 1] == T
    X = np.fft.rfft(u, n=N, axis=1)[:, j0:j0 + F]                     # (S,F,K,2)
    want = np.moveaxis((4.0 / (W * W))[:, None] * (np.abs(X) ** 2).sum(-1), 1, 2)
    worst = float((np.abs(P - want) / scale[..., None]).max())
    print(f"window {window}: restatement against rfft, largest difference {worst:.2e} of the joint's scale")
    assert worst <= 1e-13
    assert (P <= scale[..., None] * (1 + 1e-12)).all()                # no bin exceeds the scale the tolerance is relative to
    assert np.array_equal(summ[..., 0], n) and np.array_equal(summ[..., 1], W)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("T,N,m", [(600, 600, 10), (300, 300, 2), (256, 256, 100)])
def test_sinusoid_at_a_bin_has_the_power_of_its_amplitude(T, N, m):
    """A linear oscillation of amplitude A at bin m >= 2: P_m = A^2 under both windows, |sqrt P - A| <= 2^-14 px (the float32 rounding
    of coordinates below 512 is 2^-15 px); Hann additionally puts A^2 / 4 into each neighbour; rectangular: peak and centroid are m."""
    A = 30.0
    c = snp.oscillation(T, N, m, A)[None, :, None, :]
    for window in (0, 1):
        P, summ, _ = snp.spectrum(c, None, 0.3, N, 1, N // 2, window)
        row, s = P[0, 0], summ[0, 0]
        assert abs(np.sqrt(row[m - 1]) - A) <= 2.0 ** -14, (window, row[m - 1])
        assert s[0] == T and s[3] == m and s[4] == row[m - 1]
        if window == 1:
            assert abs(np.sqrt(row[m - 2]) - A / 2) <= 2.0 ** -14 and abs(np.sqrt(row[m]) - A / 2) <= 2.0 ** -14
            assert abs(s[1] - T / 2) <= 1e-9 and abs(s[2] - 1.5 * A * A) <= 1e-2
        else:
            assert s[1] == T and abs(s[5] - m) <= 1e-6 and abs(s[2] - A * A) <= 1e-2
            assert np.delete(row, m - 1).max() <= 1e-6              # the rounding of the inputs is all that is left elsewhere


def test_circle_has_twice_the_square_of_its_radius():
    T = N = 400
    R, m = 25.0, 7
    for window in (0, 1):
        P, summ, _ = snp.spectrum(snp.circle(T, N, m, R)[None, :, None, :], None, 0.3, N, 1, N // 2, window)
        assert abs(P[0, 0, m - 1] - 2 * R * R) <= 2 * 2 * R * 2.0 ** -14 and summ[0, 0, 3] == m


def test_constant_trajectory_and_single_frame_have_no_power():
    """Rectangular: sums of multiples of 1/4 are exact, so m == p.  Hann: w_t p rounds unless p is a power of two, for which
    sum (w_t p) == p sum w_t bit for bit in any one order of summation, so again m == p and every u_t is exactly 0."""
    for window, point in ((0, (100.25, 50.5)), (1, (128.0, 64.0))):
        still = np.tile(np.array([[point]], F32), (64, 1, 1))[None]
        P, summ, _ = snp.spectrum(still, None, 0.3, 128, 1, 64, window)
        assert not P.any() and summ[0, 0].tolist()[2:] == [0.0, -1.0, 0.0, 0.0] and summ[0, 0, 0] == 64
    one = np.full((1, 50, 2, 2), np.nan, F32)
    one[0, 20, 0] = (3.0, 4.0)
    one[0, :, 1] = snp.oscillation(50, 50, 5)
    P, summ, _ = snp.spectrum(one, None, 0.3, 50, 1, 25, 1)
    assert not P[0, 0].any() and summ[0, 0].tolist() == [1.0, float(snp.window_weights(50, 1)[20]), 0.0, -1.0, 0.0, 0.0]
    assert summ[0, 1, 3] == 5
    none = np.full((1, 50, 1, 2), np.nan, F32)
    assert snp.spectrum(none, None, 0.3, 50, 1, 25, 0)[1][0, 0].tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0]


def test_summary_takes_the_lowest_of_equal_maxima():
    P = np.array([[0.0, 2.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0]])
    s = snp.summary(P, np.array([9.0, 9.0]), np.array([4.5, 4.5]), 7)
    assert s[0].tolist() == [9.0, 4.5, 5.0, 8.0, 2.0, (8 * 2.0 + 9 * 1.0 + 10 * 2.0) / 5.0] and s[1].tolist() == [9.0, 4.5, 0.0, -1.0, 0.0, 0.0]


def test_phase_is_reduced_in_64_bit_integers():
    """j0 = 2^29 - 300, N = 2^30, T = 300: (j0 + j) t passes 2^32; the angles lie in [0, 2 pi) and equal the exact rational.  With that N,
    a power of two, a product that wrapped at 2^32 as an UNSIGNED number would still reduce to the same r (a signed one would not);
    N = 10^9 with j0 = 5 10^8 - 300 shows either kind, so the device tests run both."""
    for N, j0 in ((1 << 30, (1 << 29) - 300), (10 ** 9, 5 * 10 ** 8 - 300)):
        F = T = 300
        ang = snp.angles(T, N, j0, F)
        assert (j0 + F - 1) * (T - 1) > 1 << 32 and ang.min() >= 0 and ang.max() < 2 * np.pi
        for t, j in ((299, 299), (150, 7), (1, 0)):
            assert ang[t, j] == snp.TWO_PI * (float(((j0 + j) * t) % N) / float(N))
        prod = np.arange(j0, j0 + F, dtype=np.int64)[None] * np.arange(T, dtype=np.int64)[:, None]
        signed = prod.astype(np.int32).astype(np.int64)
        assert ((prod & 0xffffffff) % N != prod % N).any() == (N == 10 ** 9)
        assert (np.fmod(signed, N) != prod % N).any()


def test_quick_start_wrists_move_at_half_a_hertz():
    """The reference's clinical example (examples/quick_start.py:221-237): 200 frames over 10 s, both wrists at 0.5 Hz."""
    seq = mnp.quick_start_wrists(200)
    fps, T = 20.0, 200
    j0, F = snp.band_bins(fps, T)
    assert (j0, F) == (1, 100)
    _, summ, _ = snp.spectrum(seq[None], None, 0.3, T, j0, F, 1)
    for k in (0, 1):
        assert abs(summ[0, k, 3] / T * fps - 0.5) <= fps / T, summ[0, k]
        assert abs(np.sqrt(summ[0, k, 4]) - 30.0 * np.sqrt(2.0)) <= 1.5              # a circle of radius 30: 2 R^2, less a little leakage


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entry_is_declared_and_checks_its_arguments():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    assert "pk_motion_spectrum" in decl and len(decl["pk_motion_spectrum"][1]) == 13 and hasattr(_lib.lib, "pk_motion_spectrum")
    L, p = _lib.lib, 64                                           # a non-null pointer value that is never dereferenced: the checks refuse first

    def refused(word, coords=p, conf=None, power=p, summary=p, S=1, T=300, K=3, N=512, j0=1, F=256, window=1):
        rc = L.pk_motion_spectrum(coords, conf, power, summary, S, T, K, 0.3, N, j0, F, window, None)
        msg = L.pk_last_error_string()
        assert rc == -1 and msg.startswith(b"pk_motion_spectrum") and word in msg, (rc, msg)

    refused(b"null pointer", coords=None)
    refused(b"null pointer", power=None)
    refused(b"null pointer", summary=None)
    refused(b"j0=0", j0=0)
    refused(b"beyond N / 2", j0=2, F=256)
    refused(b"beyond N / 2", j0=2 ** 31 - 1, F=2, N=1 << 30)
    refused(b"0 bins", F=0)
    refused(b"16385 bins", F=16385, N=1 << 20)
    refused(b"N=1 ", N=1, F=1)
    refused(b"N=1073741825", N=(1 << 30) + 1)
    refused(b"window 2", window=2)
    refused(b"bad shape", T=0)
    refused(b"bad shape", K=0)


def test_op_layer_refuses_bad_arguments_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z = torch.zeros
    with pytest.raises(ValueError, match="coords"):
        hipops.motion_spectrum(z(5, 3, 2))
    with pytest.raises(ValueError, match="conf"):
        hipops.motion_spectrum(z(1, 5, 3, 2), z(1, 5, 4))
    with pytest.raises(PoseKernelError):
        hipops.motion_spectrum(z(1, 50, 3, 2))                    # a host tensor: no CPU implementation


# ------------------------------------------------------------------------------------------------ public functions
def test_movement_spectrum_names_the_band_and_the_nyquist_frequency():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    from infantposeestimation_gaussianbias_amd.utils import metrics
    seq = mnp.quick_start_wrists(200)
    with pytest.raises(ValueError, match=r"\[0\.5, 12\] Hz.*fps / 2 = 10 Hz"):
        utils.movement_spectrum(seq, 20.0, f_min=0.5, f_max=12.0)
    with pytest.raises(ValueError, match=r"\[0\.51, 0\.59\] Hz holds no bin.*fps / 2 = 10 Hz"):
        utils.movement_spectrum(seq, 20.0, f_min=0.51, f_max=0.59)
    with pytest.raises(ValueError, match="f_min"):
        utils.movement_spectrum(seq, 20.0, f_min=3.0, f_max=1.0)
    with pytest.raises(ValueError, match="window"):
        utils.movement_spectrum(seq, 20.0, window="hamming")
    with pytest.raises(ValueError, match="sequence"):
        utils.movement_spectrum(seq[0], 20.0)
    with pytest.raises(ValueError, match="fps"):
        utils.movement_spectrum(seq, 0.0)
    with pytest.raises(ValueError, match="n_fft"):
        utils.movement_spectrum(seq[:1], 20.0)
    # the bins of a band are chosen on the very frequencies that are reported
    for fps, n_fft, lo, hi in ((20.0, 200, 0.5, 3.0), (30.0, 300, 0.5, 3.0), (29.97, 1024, 0.1, 14.9), (25.0, 257, None, 2.0), (30.0, 512, 1.5, None),
                               (30.0, 300, 1.5, 1.5)):
        assert metrics._band_bins(fps, n_fft, lo, hi) == snp.band_bins(fps, n_fft, lo, hi), (fps, n_fft, lo, hi)
    assert metrics._band_bins(20.0, 200, None, None) == (1, 100) and metrics._band_bins(20.0, 201, None, None) == (1, 100)
    with pytest.raises(ValueError, match="needs fps"):
        utils.movement_report(seq, spectrum=(0.5, 3.0))
    with pytest.raises(ValueError, match="spectrum"):
        utils.movement_report(seq, spectrum=(3.0,), fps=20.0)
    with pytest.raises(ValueError, match=r"fps / 2 = 10 Hz"):
        utils.movement_report(seq, spectrum=(0.5, 30.0), fps=20.0)
    if not torch.cuda.is_available():
        for call in (lambda: utils.movement_spectrum(seq, 20.0), lambda: utils.movement_spectrum(torch.from_numpy(seq), 20.0),
                     lambda: utils.movement_report(seq, spectrum=(0.5, 3.0), fps=20.0)):
            with pytest.raises(PoseKernelError):
                call()


def test_report_without_a_spectrum_is_unchanged_and_gains_the_entries_with_one():
    """`_report_from_stats` on a stubbed (K,11) array: the keys of the report, of a joint and of a pair are today's; the spectrum entries
    come from the (K,6) summary alone."""
    from infantposeestimation_gaussianbias_amd.utils import metrics
    st = np.zeros((3, 11))
    st[:, 0], st[:, 5], st[:, 6], st[:, 7], st[:, 8], st[:, 9], st[:, 10] = 100, (60.0, 50.0, 2.0), 300.0, 99, 4.0, 10.0, 98
    rep = metrics._report_from_stats(st, 100, [(0, 1)], 5.0, 200.0, 0.2, 20.0)
    assert list(rep) == ["num_frames", "fps", "speed_unit", "temporal_consistency", "joints", "pairs"]
    assert list(rep["joints"][0]) == ["joint", "amplitude", "path_length", "mean_speed", "max_speed", "valid_fraction", "flag"]
    assert list(rep["pairs"][0]) == ["left", "right", "ratio", "asymmetric"]
    assert [j["flag"] for j in rep["joints"]] == [None, None, "low"]
    plain = json.loads(json.dumps(rep))
    summ = np.array([[100, 50, 1350.0, 5, 900.0, 5.0], [100, 50, 1000.0, 7, 625.0, 6.5], [1, 0.3, 0.0, -1, 0.0, 0.0]])
    out = metrics._add_spectrum_to_report(rep, summ, (0.5, 3.0), 100, 20.0)
    assert json.loads(json.dumps(out)) == out and out["frequency_band"] == [0.5, 3.0]
    got = [(j["dominant_frequency"], j["peak_amplitude"], j["band_power"]) for j in out["joints"]]
    assert got == [(1.0, 30.0, 1350.0), (7 / 100 * 20.0, 25.0, 1000.0), (None, 0.0, 0.0)]
    assert abs(out["pairs"][0]["frequency_difference"] - 0.4) <= 1e-12
    for key in ("dominant_frequency", "peak_amplitude", "band_power"):
        for j in out["joints"]:
            del j[key]
    del out["pairs"][0]["frequency_difference"], out["frequency_band"]
    assert out == plain


# ------------------------------------------------------------------------------------------------ config and command line
def test_yaml_frequency_band_and_its_bad_values(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.configs.config import Config
    fields = [f.name for f in dataclasses.fields(Config)]
    assert fields == ["data", "model", "train", "exp_name", "seed"] and Config.frequency_band is None and get_config().frequency_band is None

    def y(text):
        p = tmp_path / "legacy.yaml"
        p.write_text(text)
        return str(p)

    cfg = get_config(y("CLINICAL:\n  FREQUENCY_BAND: [0.5, 3]\n"))
    assert cfg.frequency_band == (0.5, 3.0) and cfg.clinical is None and Config.frequency_band is None
    assert set(dataclasses.asdict(cfg)) == set(fields)
    both = get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: true\n  FREQUENCY_BAND: [0, 2.5]\n"))
    assert both.frequency_band == (0.0, 2.5) and both.clinical["min_movement"] == 5.0
    assert get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: true\n")).frequency_band is None
    for bad in ("[3, 0.5]", "[1]", "[1, 2, 3]", "2.0", "[-1, 2]", "[a, b]", "[1, .inf]", "[true, 2]", "[1, 1]"):
        with pytest.raises(ValueError, match=r"CLINICAL\.FREQUENCY_BAND"):
            get_config(y(f"CLINICAL:\n  FREQUENCY_BAND: {bad}\n"))


def test_freq_band_without_fps_is_a_command_line_error(capsys):
    import inference
    args = inference.build_parser().parse_args(["--input", "frames", "--sequence", "--freq_band", "0.5", "3"])
    assert args.freq_band == [0.5, 3.0] and args.fps is None
    with pytest.raises(SystemExit) as e:
        inference.main(args)
    assert e.value.code == 2 and "--freq_band" in capsys.readouterr().err
    assert inference.build_parser().parse_args(["--input", "frames"]).freq_band is None
