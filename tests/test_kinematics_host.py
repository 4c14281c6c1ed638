"""Limb kinematics without a GPU: the entries' declarations and argument checks (which run before anything touches a device), the numpy
restatement (tests/kinematics_np.py) against closed forms, the margin of the cross-correlation bound between two orders of summation, the
ValueErrors of the public functions, the command line and the legacy-yaml keys.  The library functions themselves raise without a device, so
nothing here calls them past their argument checks."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import kinematics_np as knp

F32 = np.float32


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entries_and_constants_are_declared():
    from infantposeestimation_gaussianbias_amd import _lib
    decl, p, i, f = _lib.declared_symbols(), ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {"pk_joint_angles": [p, p, p, p, i, i, i, i, f, p], "pk_joint_speeds": [p, p, p, i, i, i, f, p],
            "pk_series_stats": [p, p, i, i, i, p], "pk_series_xcorr": [p, p, p, p, p, i, i, i, i, i, i, p],
            "pk_sample_entropy_tiles": [i, i], "pk_sample_entropy": [p, p, p, p, i, i, i, i, p]}
    for name, args in want.items():
        assert name in decl and decl[name] == ("int", args) and hasattr(_lib.lib, name), name
    C = _lib.CONSTANTS
    assert (C["PK_KIN_MAX_ANGLES"], C["PK_KIN_MAX_LAG"], C["PK_KIN_MAX_M"], C["PK_KIN_MAX_T"], C["PK_KIN_STATS_COLS"]) == (64, 4096, 4, 262144, 8)
    assert 64 <= C["PK_KIN_ENTROPY_TILE"] <= 256


def _refuser(name, defaults):
    from infantposeestimation_gaussianbias_amd import _lib
    L = _lib.lib

    def refused(word, code=-1, **kw):
        args = dict(defaults, **kw)
        rc = getattr(L, name)(*args.values(), None)
        msg = L.pk_last_error_string()
        assert rc == code and msg.startswith(name.encode()) and word in msg, (kw, rc, msg)
    return refused


def test_every_entry_refuses_in_the_documented_order():
    """A non-null pointer value that is never dereferenced: null first, then the shape, then the entry's own limits."""
    p = 64
    r = _refuser("pk_joint_angles", dict(coords=p, conf=None, triples=p, angles=p, S=1, T=10, K=17, A=8, min_conf=0.3))
    for arg in ("coords", "triples", "angles"):
        r(b"null pointer", **{arg: None})
    r(b"null pointer", coords=None, T=0, A=0)
    r(b"bad shape", T=0, A=0)
    r(b"bad shape", K=0)
    r(b"0 angles", A=0)
    r(b"65 angles", A=65)
    r = _refuser("pk_joint_speeds", dict(coords=p, conf=None, speeds=p, S=1, T=10, K=17, min_conf=0.3))
    r(b"null pointer", coords=None)
    r(b"null pointer", speeds=None, S=0)
    r(b"bad shape", S=0)
    r = _refuser("pk_series_stats", dict(series=p, stats=p, S=1, T=10, Q=3))
    r(b"null pointer", series=None)
    r(b"null pointer", stats=None, Q=0)
    r(b"bad shape", Q=0)
    r = _refuser("pk_series_xcorr", dict(series=p, pairs=p, corr=p, count=p, summary=p, S=1, T=10, Q=3, P=2, max_lag=4, min_count=2))
    for arg in ("series", "pairs", "corr", "count", "summary"):
        r(b"null pointer", **{arg: None})
    r(b"null pointer", corr=None, T=0, max_lag=-1)
    r(b"bad shape", T=0, max_lag=-1)
    r(b"0 pairs", P=0, max_lag=-1)
    r(b"max_lag -1", max_lag=-1, min_count=1)
    r(b"max_lag 4097", max_lag=4097)
    r(b"min_count 1", min_count=1)
    r(b"exceed one launch", code=-2, S=1 << 15, P=1 << 15, max_lag=1)
    r = _refuser("pk_sample_entropy", dict(series=p, tol=p, workspace=p, counts=p, S=1, T=100, Q=3, m=2))
    for arg in ("series", "tol", "workspace", "counts"):
        r(b"null pointer", **{arg: None})
    r(b"null pointer", tol=None, T=0, m=0)
    r(b"bad shape", T=0, m=0)
    r(b"m=0", m=0, T=1 << 20)
    r(b"m=5", m=5)
    r(b"T=262145", code=-2, T=262145)
    r(b"exceed one launch", code=-2, S=1 << 14, T=262144, Q=1)


def test_the_tile_query_counts_the_block_pairs():
    from infantposeestimation_gaussianbias_amd import _lib
    L, B0 = _lib.lib, _lib.CONSTANTS["PK_KIN_ENTROPY_TILE"]
    for T, m in ((0, 2), (-5, 2), (2, 2), (1, 1), (3, 0), (3, 5), (262145, 2)):
        assert L.pk_sample_entropy_tiles(T, m) == 0, (T, m)
    for n, nb in ((1, 1), (B0 - 1, 1), (B0, 1), (B0 + 1, 2), (2 * B0 + 1, 3), (3 * B0 + 5, 4)):
        for m in (1, 2, 4):
            assert L.pk_sample_entropy_tiles(n + m, m) == nb * (nb + 1) // 2 == knp.entropy_tiles(n + m, m, B0), (n, m)
    assert L.pk_sample_entropy_tiles(140003, 2) > 65535 and L.pk_sample_entropy_tiles(262144, 1) == 1024 * 1025 // 2


def test_op_layer_refuses_bad_arguments_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z, tri = torch.zeros, [(5, 7, 9)]
    d = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(ValueError, match="coords"):
        hipops.joint_angles(z(5, 17, 2), None, 0.3, tri)
    with pytest.raises(ValueError, match="conf"):
        hipops.joint_angles(z(1, 5, 17, 2), z(1, 5, 16), 0.3, tri)
    for bad, word in (([(5, 7, 17)], "0 to 16"), ([(5, -1, 9)], "0 to 16"), ([(5, 5, 9)], "middle joint"), ([(5, 9, 9)], "middle joint"),
                      ([(5, 7)], "3 integer"), ([], "3 integer"), ([(0.5, 1.0, 2.0)], "3 integer"), ([(0, 1, 2)] * 65, "1 to 64")):
        with pytest.raises(ValueError, match=word):
            hipops.joint_angles(z(1, 5, 17, 2), None, 0.3, bad)
    with pytest.raises(ValueError, match="coords"):
        hipops.joint_speeds(z(5, 17, 2))
    with pytest.raises(ValueError, match="series"):
        hipops.series_stats(d(5, 3))
    for kw, word in ((dict(pairs=[(0, 3)]), "0 to 2"), (dict(pairs=[(0, 1, 2)]), "2 integer"), (dict(max_lag=4097), "max_lag"),
                     (dict(max_lag=-1), "max_lag"), (dict(min_count=1), "min_count")):
        with pytest.raises(ValueError, match=word):
            hipops.series_xcorr(d(1, 9, 3), **dict(dict(pairs=[(0, 1)], max_lag=2), **kw))
    with pytest.raises(ValueError, match="tol"):
        hipops.sample_entropy_counts(d(1, 9, 3), d(1, 2))
    for m in (0, 5):
        with pytest.raises(ValueError, match="m:"):
            hipops.sample_entropy_counts(d(1, 9, 3), d(1, 3), m)
    # host tensors: no CPU implementation
    for call in (lambda: hipops.joint_angles(z(1, 5, 17, 2), None, 0.3, tri), lambda: hipops.joint_speeds(z(1, 5, 17, 2)),
                 lambda: hipops.series_stats(d(1, 5, 3)), lambda: hipops.series_xcorr(d(1, 9, 3), [(0, 1)], 2),
                 lambda: hipops.sample_entropy_counts(d(1, 9, 3), d(1, 3))):
        with pytest.raises(PoseKernelError):
            call()


# ------------------------------------------------------------------------------------------------ closed forms: angles and speeds
def test_angle_closed_forms():
    """A right angle; collinear points give exactly 0 (the rays coincide) and exactly pi (they oppose); a joint on the middle one gives NaN,
    as does a joint that is not finite or below the confidence threshold."""
    c = np.zeros((1, 6, 3, 2), F32)
    c[0, :, 1] = (10.0, 20.0)                                     # the middle joint
    c[0, 0, 0], c[0, 0, 2] = (10.0, 25.0), (17.0, 20.0)           # perpendicular rays
    c[0, 1, 0], c[0, 1, 2] = (13.0, 24.0), (16.0, 28.0)           # same direction
    c[0, 2, 0], c[0, 2, 2] = (13.0, 24.0), (4.0, 12.0)            # opposite directions
    c[0, 3, 0], c[0, 3, 2] = (10.0, 20.0), (4.0, 12.0)            # a on b
    c[0, 4, 0], c[0, 4, 2] = (13.0, 24.0), (np.nan, 12.0)
    c[0, 5, 0], c[0, 5, 2] = (13.0, 24.0), (4.0, 12.0)
    conf = np.ones((1, 6, 3), F32)
    conf[0, 5, 1] = 0.29
    th = knp.joint_angles(c, conf, 0.3, [(0, 1, 2), (2, 1, 0)])[0]
    assert th[0, 0] == np.pi / 2 and th[1, 0] == 0.0 and th[2, 0] == np.pi and np.isnan(th[3:, 0]).all()
    assert np.array_equal(th[:, 0], th[:, 1], equal_nan=True)
    assert np.array_equal(knp.joint_angles(c, None, 0.3, [(0, 1, 2)])[0, 5], [np.pi])
    sp = knp.joint_speeds(c, conf, 0.3)[0]
    assert sp[1, 2] == 20.0 and sp[0, 1] == 0.0 and np.isnan(sp[-1]).all() and np.isnan(sp[3, 2]) and np.isnan(sp[4, 2]) and np.isnan(sp[4, 1])


def test_series_stats_closed_form():
    x = np.array([1.0, 3.0, np.nan, 2.0, 6.0, np.inf, 0.0])[None, :, None]
    for order in ("ascending", "tree"):
        st = knp.series_stats(x, order=order)[0, 0]
        assert st[[0, 1, 2, 5, 6, 7]].tolist() == [5.0, 0.0, 6.0, 6.0, 2.0, 4.0]
        assert abs(st[3] - 2.4) <= 1e-15 and abs(st[4] - np.sqrt(21.2 / 5)) <= 1e-15
    assert knp.series_stats(np.full((1, 4, 1), np.nan))[0, 0].tolist() == [0.0] * 8
    assert knp.series_stats(x, mean=np.array([[2.0]]))[0, 0, 3] == 2.0


# ------------------------------------------------------------------------------------------------ closed forms: cross-correlation
def test_a_shifted_copy_peaks_at_its_shift():
    g = np.random.default_rng(1)
    a = g.standard_normal(200)
    b = np.full(200, np.nan)
    b[5:] = a[:-5]                                                # b repeats a five frames later: a leads
    corr, count = knp.xcorr(np.stack([a, b], -1)[None], [(0, 1), (1, 0)], 12)
    summ = knp.xcorr_summary(corr, count)[0]
    assert summ[0, 1] == 5 and abs(summ[0, 2] - 1.0) <= 1e-12 and summ[0, 3] == 195 and count[0, 0, 12] == 195 and count[0, 0, 0] == 183
    assert summ[1, 1] == -5 and abs(summ[1, 2] - 1.0) <= 1e-12
    assert np.array_equal(corr[0, 0], corr[0, 1][::-1]) and np.array_equal(count[0, 0], count[0, 1][::-1])


def test_constant_series_and_starved_lags_give_zero():
    T = 20
    x = np.stack([np.full(T, 3.5), np.arange(T, dtype=float), np.full(T, np.nan)], -1)[None]
    x[0, 0, 2] = x[0, 19, 2] = 1.0                                 # series 2: two valid elements, 19 frames apart
    corr, count = knp.xcorr(x, [(0, 1), (1, 1), (2, 2), (1, 2)], T + 3)
    L = T + 3
    assert not corr[0, 0].any() and count[0, 0, L] == T           # a constant has no variance: r = 0 at every lag
    assert count[0, 1, L + T - 1] == 1 and corr[0, 1, L + T - 1] == 0 and count[0, 1, L + T] == 0 and corr[0, 1, L + T:].tolist() == [0.0] * 4
    assert abs(corr[0, 1, L] - 1.0) <= 1e-15 and count[0, 1, L + T - 2] == 2
    assert count[0, 2, L] == 2 and corr[0, 2, L] == 0.0 and count[0, 2, L + 19] == 1 and count[0, 2, L + 1] == 0     # (1, 1): sxx = 0
    summ = knp.xcorr_summary(corr, count, 3)[0]
    assert summ[2].tolist() == [0.0, 0.0, 0.0, 0.0]               # no lag of (2, 2) has three pairs
    assert summ[1, 0] == corr[0, 1, L] and summ[1, 3] >= 3
    flat = knp.xcorr_summary(np.array([0.5, 0.9, 0.9, 0.1, 0.95]), np.array([5, 5, 5, 5, 1]), 2)
    assert flat.tolist() == [0.9, -1.0, 0.9, 5.0]                 # the lowest of equal maxima; the starved lag never wins


def test_the_xcorr_bound_holds_between_ascending_and_tree_order():
    """|dr| <= (n + 16) 2^-50 is derived for any order of the n-term sums; here the two orders the tests meet (a running sum and the
    device's tree) are compared at the largest length the device test uses, with gaps."""
    x = knp.series_case(2, 513, 4, seed=4)
    pairs = [(0, 3), (3, 0), (0, 0), (3, 2)]
    ra, na = knp.xcorr(x, pairs, 40, "ascending")
    rt, nt = knp.xcorr(x, pairs, 40, "tree")
    assert np.array_equal(na, nt)
    share = float((np.abs(ra - rt) / ((na + 16) * 2.0 ** -50)).max())
    print(f"xcorr, ascending against tree order: largest difference {share:.3e} of the bound")
    assert share <= 1.0 and np.array_equal(rt[:, 0], rt[:, 1][:, ::-1])


# ------------------------------------------------------------------------------------------------ closed forms: sample entropy
def test_entropy_counts_closed_forms():
    n, m = 57, 2
    assert knp.entropy_counts_1d(np.full(n + m, 4.0), 0.0, m) == (n, n * (n - 1) // 2, n * (n - 1) // 2)
    assert knp.entropy_counts_1d(np.arange(n + m) * 0.5, 0.4999, m) == (n, 0, 0)
    tol = 0.3
    tie = np.array([0.0, tol, 0.0, tol, 0.0])                     # |0 - tol| == tol: equality is a match, so every pair matches
    assert knp.entropy_counts_1d(tie, tol, 1) == (4, 6, 6)
    above = np.array([0.0, np.nextafter(tol, 1.0), 0.0, np.nextafter(tol, 1.0), 0.0])
    assert knp.entropy_counts_1d(above, tol, 1) == (4, 2, 2)      # one ulp above does not: only like matches like
    assert knp.entropy_counts_1d(np.array([0.0, 0.0, 0.0, tol, 0.0, np.nextafter(tol, 1.0)]), tol, 2) == (4, 6, 4)
    for bad in (-1.0, np.nan, np.inf):
        assert knp.entropy_counts_1d(np.zeros(10), bad, 2) == (8, 0, 0)
    gap = np.zeros(10)
    gap[4] = np.nan                                               # starts 2, 3, 4 reach the gap (m = 2)
    assert knp.template_starts(gap, 2).tolist() == [0, 1, 5, 6, 7] and knp.entropy_counts_1d(gap, 0.0, 2) == (5, 10, 10)
    assert knp.entropy_counts_1d(np.zeros(2), 0.1, 2) == (0, 0, 0) and knp.sample_entropy((5, 0, 0)) is None


def test_a_sine_is_simpler_than_noise():
    """SampEn(2, 0.2) of a sine of period 37 over 700 frames against seeded white noise (a prototype of these definitions gave 0.22 and 2.28)."""
    T = 700
    x = np.stack([np.sin(2 * np.pi * np.arange(T) / 37.0), np.random.default_rng(0).standard_normal(T)], -1)[None]
    tol = knp.series_stats(x)[..., 4] * 0.2
    counts = knp.sample_entropy_counts(x, tol, 2)[0]
    sine, noise = knp.sample_entropy(counts[0]), knp.sample_entropy(counts[1])
    print(f"sample entropy: sine {sine:.3f}, noise {noise:.3f}")
    assert counts[0, 0] == counts[1, 0] == T - 2 and sine < 0.5 < 1.5 < noise


# ------------------------------------------------------------------------------------------------ public functions
def test_public_functions_check_before_they_need_a_device():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    assert list(utils.COCO_ANGLES.items()) == list(knp.COCO_ANGLES.items()) and list(utils.COCO_ANGLES)[0] == "left_elbow"
    seq13, seq17 = np.zeros((20, 13, 2), F32), np.zeros((20, 17, 2), F32)
    with pytest.raises(ValueError, match=r"13 joints has no default.*angles="):
        utils.kinematics_report(seq13)
    with pytest.raises(ValueError, match=r"13 joints has no default.*angles="):
        utils.joint_angle_series(seq13)
    with pytest.raises(ValueError, match=r"angles\['knee'\]"):
        utils.kinematics_report(seq13, angles={"knee": (7, 9, 13)})
    with pytest.raises(ValueError, match="sequence"):
        utils.kinematics_report(seq17[0])
    with pytest.raises(ValueError, match="max_lag"):
        utils.kinematics_report(seq17, max_lag=-1)
    with pytest.raises(ValueError, match="entropy m"):
        utils.kinematics_report(seq17, entropy=(5, 0.2))
    with pytest.raises(ValueError, match="entropy r"):
        utils.kinematics_report(seq17, entropy=(2, -0.1))
    with pytest.raises(ValueError, match="flip_pairs"):
        utils.kinematics_report(seq17, flip_pairs=[(1, 17)])
    with pytest.raises(ValueError, match="kinematics takes a dict"):
        utils.movement_report(seq17, kinematics={"lag": 3})
    with pytest.raises(ValueError, match="one length"):
        utils.limb_coordination(np.zeros(5), np.zeros(6), 2)
    with pytest.raises(ValueError, match="m must be"):
        utils.sample_entropy(np.zeros(50), m=0)
    if not torch.cuda.is_available():
        for call in (lambda: utils.kinematics_report(seq17), lambda: utils.kinematics_report(torch.from_numpy(seq17)),
                     lambda: utils.joint_angle_series(seq13, angles={"knee": (7, 9, 11)}), lambda: utils.sample_entropy(np.zeros(50)),
                     lambda: utils.limb_coordination(np.zeros(9), np.zeros(9), 2), lambda: utils.movement_report(seq17, kinematics={})):
            with pytest.raises(PoseKernelError):
                call()


# ------------------------------------------------------------------------------------------------ config and command line
def test_yaml_keys_fill_their_own_attributes(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.configs.config import Config
    fields = [f.name for f in dataclasses.fields(Config)]
    assert fields == ["data", "model", "train", "exp_name", "seed"] and Config.joint_angles is None and Config.kinematics is None

    def y(text):
        p = tmp_path / "legacy.yaml"
        p.write_text(text)
        return str(p)

    plain = get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: true\n"))
    cfg = get_config(y("CLINICAL:\n  ENABLE_MOVEMENT_TRACKING: true\n  JOINT_ANGLES:\n    left_knee: [7, 9, 11]\n    right_knee: [8, 10, 12]\n"
                       "  KINEMATICS: {MAX_LAG: 45, ENTROPY_M: 3, ENTROPY_R: 0.15}\n"))
    assert cfg.joint_angles == {"left_knee": (7, 9, 11), "right_knee": (8, 10, 12)} and list(cfg.joint_angles) == ["left_knee", "right_knee"]
    assert cfg.kinematics == {"max_lag": 45, "entropy": (3, 0.15)}
    assert cfg.clinical == plain.clinical and plain.joint_angles is None and plain.kinematics is None and Config.kinematics is None
    assert set(dataclasses.asdict(cfg)) == set(fields)
    assert get_config(y("CLINICAL:\n  KINEMATICS: {ENTROPY_R: 0.25}\n")).kinematics == {"max_lag": None, "entropy": (2, 0.25)}
    for text, key in (("JOINT_ANGLES: [1, 2, 3]", r"CLINICAL\.JOINT_ANGLES"), ("JOINT_ANGLES: {knee: [1, 1, 3]}", r"CLINICAL\.JOINT_ANGLES\['knee'\]"),
                      ("JOINT_ANGLES: {knee: [1, 2]}", r"CLINICAL\.JOINT_ANGLES\['knee'\]"), ("JOINT_ANGLES: {knee: [1, -2, 3]}", r"CLINICAL\.JOINT_ANGLES"),
                      ("KINEMATICS: {MAX_LAG: -1}", r"CLINICAL\.KINEMATICS\.MAX_LAG"), ("KINEMATICS: {MAX_LAG: 1.5}", r"CLINICAL\.KINEMATICS\.MAX_LAG"),
                      ("KINEMATICS: {ENTROPY_M: 5}", r"CLINICAL\.KINEMATICS\.ENTROPY_M"), ("KINEMATICS: {ENTROPY_R: -0.2}", r"CLINICAL\.KINEMATICS\.ENTROPY_R"),
                      ("KINEMATICS: {ENTROPY_R: .nan}", r"CLINICAL\.KINEMATICS\.ENTROPY_R"), ("KINEMATICS: {LAG: 3}", r"CLINICAL\.KINEMATICS"),
                      ("KINEMATICS: 7", r"CLINICAL\.KINEMATICS")):
        with pytest.raises(ValueError, match=key):
            get_config(y(f"CLINICAL:\n  {text}\n"))


def test_the_parser_takes_the_flags_and_refuses_them_without_a_sequence(capsys):
    import inference
    parse = inference.build_parser().parse_args
    args = parse(["--input", "frames", "--sequence", "--kinematics", "--max_lag", "45", "--entropy", "3", "0.15"])
    assert args.kinematics is True and args.max_lag == 45 and args.entropy == [3.0, 0.15]
    plain = parse(["--input", "frames", "--sequence"])
    assert plain.kinematics is False and plain.max_lag is None and plain.entropy is None
    for argv, word in ((["--kinematics"], "needs --sequence"), (["--sequence", "--max_lag", "5"], "belong to --kinematics"),
                       (["--sequence", "--kinematics", "--max_lag", "5000"], "--max_lag"),
                       (["--sequence", "--kinematics", "--entropy", "5", "0.2"], "--entropy"),
                       (["--sequence", "--kinematics", "--entropy", "2.5", "0.2"], "--entropy")):
        with pytest.raises(SystemExit) as e:
            parse(["--input", "frames"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    cfg = type("Cfg", (), {"joint_angles": {"knee": (1, 2, 3)}, "kinematics": {"max_lag": 45, "entropy": (3, 0.15)}})()
    assert inference._kinematics_settings(cfg, None) is None and inference._kinematics_settings(cfg, False) is None
    assert inference._kinematics_settings(cfg, True) == {"angles": {"knee": (1, 2, 3)}, "max_lag": 45, "entropy": (3, 0.15)}
    assert inference._kinematics_settings(cfg, {"max_lag": 7, "entropy": None}) == {"angles": {"knee": (1, 2, 3)}, "max_lag": 7, "entropy": (3, 0.15)}
    assert inference._kinematics_settings(type("Cfg", (), {})(), True) == {}
