"""The ensemble unit and the uncertainty surface without a GPU: the two entries in the header and the library, every refusal with its text
before any launch, the restatement against numpy's own mean / std / cov, the exported names, and the switches of inference.py.  The
kernels themselves raise without a device, so nothing here calls them past their argument checks."""
import numpy as np
import pytest
import torch

import ensemble_np as enp


def _err():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib.lib.pk_last_error_string().decode()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_two_entries_are_declared_with_their_argument_counts_and_limits():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_ensemble_moments", 8), ("pk_ensemble_points", 10)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(_lib.lib, name), name
    assert _lib.CONSTANTS["PK_ENS_REG_MEMBERS"] == 32 and _lib.CONSTANTS["PK_ENS_GRID_CAP"] == 4096
    assert _lib.CONSTANTS["PK_ENS_POINT_GRID_CAP"] == 65536
    assert _lib.CONSTANTS["PK_ENS_POINT_COLS"] == enp.COLS == len(hipops.ENSEMBLE_POINT_COLUMNS) == 12


def test_every_refusal_comes_back_with_its_text_before_any_launch():
    from infantposeestimation_gaussianbias_amd import _lib
    L, p = _lib.lib, 4096                                         # a non-null aligned pointer value that is never dereferenced: the checks refuse first
    far = p + (1 << 30)

    def moments(stack=p, stride=100, S=5, n=100, ddof=0, mean=far, std=far + 4096):
        return L.pk_ensemble_moments(stack, stride, S, n, ddof, mean, std, None)

    for name in ("stack", "mean", "std"):
        assert moments(**{name: None}) == -1 and _err() == "pk_ensemble_moments: null pointer", name
    assert moments(S=0) == -1 and _err() == "pk_ensemble_moments: 0 members with ddof=0 (at least 1)"
    assert moments(S=1, ddof=1) == -1 and _err() == "pk_ensemble_moments: 1 members with ddof=1 (at least 2)"
    assert moments(S=-3) == -1
    assert moments(ddof=2) == -1 and _err() == "pk_ensemble_moments: ddof 2 (0 or 1)"
    assert moments(ddof=-1) == -1
    assert moments(n=0) == -1 and _err() == "pk_ensemble_moments: bad length L=0"
    assert moments(n=-7) == -1 and _err() == "pk_ensemble_moments: bad length L=-7"
    assert moments(stride=99) == -1 and _err() == "pk_ensemble_moments: member_stride=99 below L=100"
    # the stack is (S - 1) stride + L = 500 floats = 2000 bytes: an output inside, at its last float, and ending inside its first
    for out in (p, p + 1996, p - 396):
        assert moments(mean=out) == -1 and _err() == "pk_ensemble_moments: an output overlaps the stack", out
        assert moments(std=out) == -1 and _err() == "pk_ensemble_moments: an output overlaps the stack", out
    assert moments(std=far + 396) == -1 and _err() == "pk_ensemble_moments: mean and std overlap"
    assert moments(S=2 ** 31 - 1, stride=2 ** 40, n=8) == -1 and "stack too large" in _err()

    def points(coords=p, conf=p, centre=p, out=p, S=5, M=3, min_conf=0.0, radius=1.0, ddof=0):
        return L.pk_ensemble_points(coords, conf, centre, out, S, M, min_conf, radius, ddof, None)

    for name in ("coords", "out"):
        assert points(**{name: None}) == -1 and _err() == "pk_ensemble_points: null pointer", name
    assert points(S=0) == -1 and _err() == "pk_ensemble_points: bad shape S=0 M=3"
    assert points(M=0) == -1 and _err() == "pk_ensemble_points: bad shape S=5 M=0"
    assert points(M=-2) == -1 and points(S=-1) == -1
    assert points(radius=-0.5) == -1 and _err() == "pk_ensemble_points: radius -0.5 (finite, at least 0)"
    assert points(radius=float("inf")) == -1 and _err() == "pk_ensemble_points: radius inf (finite, at least 0)"
    assert points(radius=float("nan")) == -1 and "radius" in _err()
    assert points(ddof=2) == -1 and _err() == "pk_ensemble_points: ddof 2 (0 or 1)"
    assert points(ddof=-1) == -1


def test_op_layer_refuses_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z = torch.zeros
    with pytest.raises(PoseKernelError, match="no CPU implementation"):           # host tensors
        hipops.ensemble_moments(z(4, 3, 5))
    with pytest.raises(PoseKernelError, match="no CPU implementation"):
        hipops.ensemble_points(z(4, 3, 2))
    with pytest.raises(PoseKernelError, match="ddof"):
        hipops.ensemble_moments(z(4, 3, 5), ddof=2)
    with pytest.raises(PoseKernelError, match="ddof"):
        hipops.ensemble_points(z(4, 3, 2), ddof=-1)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restated_moments_are_numpys_within_rounding_and_exact_where_the_order_cannot_matter():
    g = np.random.default_rng(1)
    for S in (1, 2, 30, 33):
        st = (g.standard_normal((S, 4, 9)) * 3 + 1).astype(np.float32)
        for ddof in (0, 1):
            if S < 1 + ddof:
                continue
            m, s = enp.moments(st, ddof)
            assert m.dtype == s.dtype == np.float32 and m.shape == s.shape == (4, 9)
            # float64 sums of S values differ from numpy's pairwise order by a few ulp of float64: far below half an ulp of float32
            assert np.allclose(m, st.astype(np.float64).mean(0), rtol=2e-7, atol=1e-7)
            assert np.allclose(s, st.astype(np.float64).std(0, ddof=ddof), rtol=2e-7, atol=1e-7)
    same = np.full((7, 5), 0.3, np.float32)
    m, s = enp.moments(same)
    assert np.array_equal(m, same[0]) and not s.any()             # S x / S is exact for S < 2^29
    st = np.ones((3, 4), np.float32)
    st[1, 0], st[2, 1] = np.nan, np.inf
    m, s = enp.moments(st)
    assert np.isnan(m[0]) and np.isnan(s[0]) and m[1] == np.inf and np.isnan(s[1]) and m[2] == 1 and s[2] == 0


def test_restated_points_are_numpys_mean_cov_and_counts():
    g = np.random.default_rng(2)
    S, M = 300, 3
    c = (g.standard_normal((S, M, 2)) * np.array([2.0, 0.5])).astype(np.float32)
    cf = g.random((S, M)).astype(np.float32)
    c[5, 0] = np.nan
    cf[7, 0] = np.inf
    centre = g.standard_normal((M, 2))
    out = enp.points(c, cf, centre, min_conf=0.25, radius=1.5, ddof=1)
    assert out.shape == (M, 12)
    for m in range(M):
        ok = np.isfinite(c[:, m]).all(1) & np.isfinite(cf[:, m]) & (cf[:, m] >= np.float32(0.25))
        xy, w = c[ok, m].astype(np.float64), cf[ok, m].astype(np.float64)
        cov = np.cov(xy.T)
        lam = np.linalg.eigvalsh(cov)[::-1]
        want = [ok.sum(), *xy.mean(0), cov[0, 0], cov[1, 1], cov[0, 1], *lam, w.mean(), w.std(ddof=1), w.min(),
                (((xy - centre[m]) ** 2).sum(1) <= 1.5 ** 2).sum()]
        assert np.allclose(out[m], want, rtol=1e-10, atol=1e-12), m
        assert out[m, 0] == want[0] and out[m, 10] == want[10] and out[m, 11] == want[11]
    none = enp.points(c, None, None, ddof=0)
    assert not none[:, 8:11].any() and none[0, 0] == S - 1 and none[1, 0] == S
    gone = enp.points(np.full((4, 2, 2), np.nan, np.float32))
    assert not gone.any()
    one = enp.points(c[:1], ddof=1)                               # n = 1 < 1 + ddof
    assert not one.any()


# ------------------------------------------------------------------------------------------------ the public surface
def test_the_names_are_exported_and_have_no_host_path():
    from infantposeestimation_gaussianbias_amd import nnops, utils
    assert {"uncertainty", "UncertaintyAnalyzer", "mc_uncertainty"} <= set(utils.__all__)
    assert callable(utils.mc_uncertainty) and callable(utils.UncertaintyAnalyzer.monte_carlo_dropout_uncertainty)
    assert "stochastic depth" in utils.UncertaintyAnalyzer.monte_carlo_dropout_uncertainty.__doc__
    model = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match="eval"):
        utils.mc_uncertainty(model.train(), torch.zeros(1, 3, 32, 24))
    with pytest.raises(ValueError, match="no stochastic-depth layer"):
        utils.mc_uncertainty(model.eval(), torch.zeros(1, 3, 32, 24))
    with nnops.stochastic_depth(rate=0.25) as sd:
        assert sd.scales is None and sd.uses == 0 and nnops.eval_drop_scales(4, 3, 0.1, torch.device("cpu")).shape == (4, 3)
        assert all(v == 0.0 or abs(v - 1 / 0.75) <= 2.0 ** -23 * (1 / 0.75) for v in sd.scales.unique().tolist()) and sd.uses == 1
        assert nnops.eval_drop_scales(0, 3, 0.1, torch.device("cpu")) is None
    assert nnops.eval_drop_scales(4, 3, 0.1, torch.device("cpu")) is None          # outside the context nothing draws
    with nnops.stochastic_depth(rate=0) as sd:
        assert nnops.eval_drop_scales(4, 3, 0.1, torch.device("cpu")) is None and sd.scales is None
    given = torch.ones(4, 3)
    with nnops.stochastic_depth(scales=given) as sd:
        assert nnops.eval_drop_scales(4, 3, 0.1, torch.device("cpu")) is sd.scales and torch.equal(sd.scales, given)
        with pytest.raises(ValueError, match="this forward takes"):
            nnops.eval_drop_scales(6, 3, 0.1, torch.device("cpu"))
    with pytest.raises(ValueError):
        nnops.stochastic_depth(rate=1.0)
    with pytest.raises(ValueError):
        nnops.stochastic_depth(scales=torch.ones(3))


def test_inference_parser_knows_the_uncertainty_switches_and_what_they_exclude():
    import inference
    p = inference.build_parser()
    args = p.parse_args(["--input", "x.png"])
    assert args.uncertainty is None and args.uncertainty_rate is None and args.uncertainty_seed == 0
    args = p.parse_args(["--input", "x.png", "--bbox", "1", "2", "3", "4", "--uncertainty", "30", "--uncertainty_rate", "0.2",
                         "--uncertainty_seed", "7", "--report", "r.json", "--output", "o.png"])
    assert (args.uncertainty, args.uncertainty_rate, args.uncertainty_seed, args.report, args.output) == (30, 0.2, 7, "r.json", "o.png")
    for extra in (["--occlusion_map", "5"], ["--sequence"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--input", "x.png", "--uncertainty", "30"] + extra)
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "x.png", "--uncertainty", "0"])
    p.parse_args(["--input", "x", "--sequence", "--report", "r.json"])              # the other switches are as they were
    assert hasattr(inference.PoseInference, "uncertainty") and callable(inference.main_uncertainty)
