"""Localisation error analysis without a GPU: the two entries in the header and their refusals, the four limits from the header to the op
layer, the host arithmetic of `KeypointErrorAnalyzer.compute()` on hand-made counters (suffix sums against the reference's tp / fp / fn
loop, the sign of AP, the calibration error, numpy's quantile rule on two order statistics), the restatement's fixed-order sum, and the
two flags of validate.py.  The library functions themselves raise without a device, so nothing here calls them past their argument checks."""
import numpy as np
import pytest
import torch

import error_analysis_np as enp

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_two_entries_are_declared_with_their_argument_counts():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_kpt_error", 18), ("pk_kpt_error_quantiles", 9)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(_lib.lib, name)


def test_the_four_limits_come_from_the_public_header():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    want = {"PK_ERR_MAX_BINS": 256, "PK_ERR_MAX_CONF_THR": 1024, "PK_ERR_MAX_QUANTILES": 16, "PK_ERR_MAX_COLS": 2 ** 31 - 1}
    assert {k: _lib.CONSTANTS.get(k) for k in want} == want
    assert (hipops.ERR_MAX_BINS, hipops.ERR_MAX_CONF_THRESHOLDS, hipops.ERR_MAX_QUANTILES, hipops.ERR_MAX_COLS) == (256, 1024, 16, 2 ** 31 - 1)


def test_every_refusal_comes_back_with_its_text():
    from infantposeestimation_gaussianbias_amd import _lib
    L, p = _lib.lib, 64                                           # a non-null pointer value that is never dereferenced: the checks refuse first
    err = lambda: L.pk_last_error_string().decode()

    names = ("pred", "gt", "vis", "conf", "norm", "bin_edges", "conf_thr", "err_out", "calib_count", "calib_hit", "pr_hist")

    def kpt_error(n_bins=10, T=100, ld=8, N=8, K=3, **ptrs):
        a = {name: ptrs.get(name, p) for name in names}
        return L.pk_kpt_error(a["pred"], a["gt"], a["vis"], a["conf"], a["norm"], 10.0, a["bin_edges"], n_bins, a["conf_thr"], T, a["err_out"], ld,
                              a["calib_count"], a["calib_hit"], a["pr_hist"], N, K, None)

    assert kpt_error(n_bins=257) == -1 and err() == "pk_kpt_error: 257 confidence bins (1 to 256)"
    assert kpt_error(n_bins=0) == -1 and err() == "pk_kpt_error: 0 confidence bins (1 to 256)"
    assert kpt_error(T=1025) == -1 and err() == "pk_kpt_error: 1025 confidence thresholds (1 to 1024)"
    assert kpt_error(T=0) == -1 and err() == "pk_kpt_error: 0 confidence thresholds (1 to 1024)"
    assert kpt_error(ld=7) == -1 and err() == "pk_kpt_error: row stride ld=7 below N=8"
    assert kpt_error(N=0, ld=0) == -1 and err() == "pk_kpt_error: bad shape N=0 K=3"
    assert kpt_error(K=0) == -1 and err() == "pk_kpt_error: bad shape N=8 K=0"
    for name in ("pred", "gt", "vis", "err_out"):                 # always required (norm and conf may be null)
        assert kpt_error(**{name: None}) == -1 and err() == "pk_kpt_error: null pointer", name
    for name in ("bin_edges", "conf_thr", "calib_count", "calib_hit", "pr_hist"):      # required with a confidence
        assert kpt_error(**{name: None}) == -1, name
        assert err() == "pk_kpt_error: null pointer (a confidence needs bin_edges, conf_thr and the three counters)", name

    def quantiles(err_p=p, q=p, order=p, summary=p, ld=100, n_cols=100, K=3, Q=5):
        return L.pk_kpt_error_quantiles(err_p, ld, n_cols, K, q, Q, order, summary, None)

    assert quantiles(Q=17) == -1 and err() == "pk_kpt_error_quantiles: 17 quantiles (1 to 16)"
    assert quantiles(Q=0) == -1 and err() == "pk_kpt_error_quantiles: 0 quantiles (1 to 16)"
    assert quantiles(ld=99) == -1 and err() == "pk_kpt_error_quantiles: row stride ld=99 below n_cols=100"
    assert quantiles(n_cols=0) == -1 and err() == "pk_kpt_error_quantiles: bad shape K=3 n_cols=0 (1 to 2147483647 columns)"
    assert quantiles(n_cols=2 ** 31, ld=2 ** 31) == -1
    assert err() == "pk_kpt_error_quantiles: bad shape K=3 n_cols=2147483648 (1 to 2147483647 columns)"
    assert quantiles(K=0) == -1 and err() == "pk_kpt_error_quantiles: bad shape K=0 n_cols=100 (1 to 2147483647 columns)"
    for name in ("err_p", "q", "order", "summary"):
        assert quantiles(**{name: None}) == -1 and err() == "pk_kpt_error_quantiles: null pointer", name


def test_op_layer_refuses_mismatched_shapes_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z = torch.zeros
    buf = hipops.kpt_error_buffers(3, 10, 100, "cpu")
    assert [tuple(b.shape) for b in buf] == [(3, 10), (3, 10), (3, 2, 101)] and all(b.dtype == torch.int64 and not b.any() for b in buf)
    store = z(3, 16)
    good = dict(pred=z(4, 3, 2), gt=z(4, 3, 2), visible=z(4, 3), store=store, column=0, pixel_threshold=10.0)
    conf = dict(confidence=z(4, 3), bin_edges=z(11), conf_thresholds=z(100), calib_count=buf[0], calib_hit=buf[1], pr_hist=buf[2])
    for bad in (dict(pred=z(4, 3, 3)), dict(gt=z(4, 2, 2)), dict(visible=z(4, 4)), dict(normalizer=z(5)), dict(store=z(2, 16)),
                dict(column=13), dict(column=-1), dict(store=z(16, 3).t()), dict(confidence=z(4, 3)), dict(conf, confidence=z(4, 2)),
                dict(conf, bin_edges=z(258)), dict(conf, bin_edges=z(1)), dict(conf, conf_thresholds=z(1025)), dict(conf, conf_thresholds=z(0)),
                dict(conf, pr_hist=z(3, 2, 100, dtype=torch.int64)), dict(conf, calib_hit=z(10, 3, dtype=torch.int64).t())):
        with pytest.raises(ValueError):
            hipops.kpt_error_accumulate(**{**good, **bad})
    with pytest.raises(PoseKernelError):                          # right shapes on the host: no CPU implementation, still no launch
        hipops.kpt_error_accumulate(**good, **conf)
    q = z(5, dtype=torch.float64)
    for bad_store, n_cols, bad_q in ((z(3), 1, q), (store, 17, q), (store, -1, q), (z(16, 3).t(), 3, q), (store, 8, z(17, dtype=torch.float64)),
                                     (store, 8, z(0, dtype=torch.float64)), (store, 8, z(1, 5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            hipops.kpt_error_quantiles(bad_store, n_cols, bad_q)
    with pytest.raises(PoseKernelError):
        hipops.kpt_error_quantiles(store, 8, q)


# ------------------------------------------------------------------------------------------------ compute()'s host arithmetic
def test_suffix_sums_equal_the_reference_loop_on_three_samples():
    """Three pairs of one joint, thresholds 0.25, 0.5, 0.75: errors 3 (correct), 12 (not), 5 (correct) at confidences 0.9, 0.6, 0.3.  By
    hand: at 0.25 all three are detected (tp 2, fp 1, fn 0); at 0.5 the first two (tp 1, fp 1, fn 1); at 0.75 the first (tp 1, fp 0, fn 1)."""
    from infantposeestimation_gaussianbias_amd.utils import metrics
    err, conf = np.array([[3.0], [12.0], [5.0]], F32), np.array([[0.9], [0.6], [0.3]], F32)
    thr = np.array([0.25, 0.5, 0.75], F32)
    tp, fp, fn = enp.pr_reference(err, conf, 10.0, thr)
    assert (tp[0].tolist(), fp[0].tolist(), fn[0].tolist()) == ([2, 1, 1], [1, 1, 0], [0, 1, 1])
    hist = enp.pr_hist(err, conf, 10.0, thr)
    assert hist[0].tolist() == [[0, 1, 0, 1], [0, 0, 1, 0]]      # m = 1 (conf 0.3), m = 3 (0.9) correct; m = 2 (0.6) not
    for got, want in zip(metrics._pr_counts(hist), (tp, fp, fn)):
        assert np.array_equal(got, want)
    for got, want in zip(enp.suffix_counts(hist), (tp, fp, fn)):
        assert np.array_equal(got, want)
    pr = metrics._precision_recall(thr, hist[0])
    precision, recall, area = enp.reference_curves(tp[0], fp[0], fn[0])
    assert np.array_equal(pr["precision"], precision) and np.array_equal(pr["recall"], recall)
    assert precision.tolist() == [2 / 3, 0.5, 1.0] and recall.tolist() == [1.0, 0.5, 0.5]
    # recall falls as the threshold rises: the reference's trapz over it is the negative area, ours its negation
    assert area == -(0.5 * (2 / 3 + 0.5) / 2) and pr["ap"] == -area and pr["ap"] > 0


def test_suffix_sums_equal_the_reference_loop_on_a_random_case():
    from infantposeestimation_gaussianbias_amd.utils import metrics
    pred, gt, vis, norm, conf, edges, thr = enp.error_case(257, 3, False, True)
    err = enp.errors(pred, gt, vis)
    hist = enp.pr_hist(err, conf, enp.PIXEL_THR, thr)
    want = enp.pr_reference(err, conf, enp.PIXEL_THR, thr)
    for got, w in zip(metrics._pr_counts(hist), want):
        assert np.array_equal(got, w)
    used = ~np.isnan(err) & np.isfinite(conf)
    assert hist.sum() == used.sum() and 0 < used.sum() < (~np.isnan(err)).sum() < err.size
    pooled = metrics._pr_counts(hist.sum(0))
    assert all(np.array_equal(p, w.sum(0)) for p, w in zip(pooled, want))
    pr = metrics._precision_recall(thr, hist.sum(0))
    precision, recall, area = enp.reference_curves(*(w.sum(0) for w in want))
    assert np.array_equal(pr["precision"], precision) and np.array_equal(pr["recall"], recall) and pr["ap"] == -area and pr["ap"] > 0
    assert pr["precision"].shape == (100,)


def test_calibration_accuracy_and_expected_calibration_error_by_hand():
    from infantposeestimation_gaussianbias_amd.utils import metrics
    edges = np.array([0.0, 0.5, 1.0], F32)
    cal = metrics._calibration(edges, [4, 0], [1, 0])
    assert cal["accuracy"].tolist() == [0.25, 0.0] and cal["ece"] == 0.0        # centre 0.25, accuracy 0.25; the empty bin has accuracy 0, weight 0
    cal = metrics._calibration(edges, [4, 12], [1, 12])
    assert cal["accuracy"].tolist() == [0.25, 1.0] and cal["ece"] == (4 * 0.0 + 12 * 0.25) / 16
    assert metrics._calibration(edges, [0, 0], [0, 0])["ece"] == 0.0
    # the default edges: a confidence of exactly 1.0 lies inside the last bin; the reference's own edges drop it
    d = metrics.default_confidence_edges(10)
    assert d.dtype == F32 and len(d) == 11 and np.array_equal(d[:-1], enp.REFERENCE_EDGES.astype(F32)[:-1]) and d[-1] == np.nextafter(F32(1), F32(2))
    err, conf = np.zeros((1, 1), F32), np.ones((1, 1), F32)
    assert enp.calibration(err, conf, 10.0, d)[0][0].tolist() == [0] * 9 + [1]
    assert enp.calibration(err, conf, 10.0, enp.REFERENCE_EDGES)[0].sum() == 0


def test_quantile_values_follow_numpy_on_the_two_order_statistics():
    from infantposeestimation_gaussianbias_amd.utils import metrics
    g = np.random.default_rng(5)
    q = enp.QUANTILES
    rows = [np.abs(g.standard_normal(n) * 6).astype(F32) for n in (1, 2, 5, 100, 257)]
    order = np.stack([enp.order_stats(r, q) for r in rows])
    n = np.array([len(r) for r in rows])
    got = metrics._quantile_values(order, n, q)
    for k, r in enumerate(rows):
        assert np.array_equal(got[k], np.quantile(r.astype(F64), q)), k
    assert np.array_equal(metrics._quantile_values(order[:, 2:3], n, np.array([0.5])), np.stack([np.percentile(r.astype(F64), [50]) for r in rows]))
    assert np.isnan(metrics._quantile_values(np.zeros((1, len(q), 2), F32), np.array([0]), q)).all()


def test_analyzer_checks_its_arguments_and_has_no_host_path():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    assert "KeypointErrorAnalyzer" in utils.__all__ and "keypoint_error_report" in utils.__all__
    a = utils.KeypointErrorAnalyzer(17)
    assert a.pixel_threshold == 10.0 and a.quantiles.tolist() == [0.05, 0.25, 0.5, 0.75, 0.95]
    assert np.array_equal(a.conf_thresholds, np.linspace(0, 1, 100).astype(F32)) and len(a.edges) == 11
    for bad in (dict(quantiles=()), dict(quantiles=[0.1] * 17), dict(quantiles=[1.5]), dict(conf_bins=0), dict(conf_bins=257),
                dict(conf_bins=[0.5, 0.1]), dict(conf_thresholds=[]), dict(conf_thresholds=np.zeros(1025)), dict(conf_thresholds=[0.5, 0.1]),
                dict(capacity=0)):
        with pytest.raises(ValueError):
            utils.KeypointErrorAnalyzer(17, **bad)
    empty = a.compute()                                           # before the first update: nothing counted, nothing launched
    assert empty["n"] == 0 and empty["ece"] == 0.0 and empty["ap"] == 0.0 and len(empty["joints"]) == 17
    assert np.isnan(empty["joints"][0]["quantiles"]).all() and not empty["calibration"]["count"].any()
    if not torch.cuda.is_available():
        with pytest.raises(PoseKernelError):
            a.update(np.zeros((2, 17, 2)), np.zeros((2, 17, 2)), np.ones((2, 17)))
        with pytest.raises(PoseKernelError):
            utils.keypoint_error_report(torch.zeros(2, 3, 2), torch.zeros(2, 3, 2), torch.ones(2, 3))


def test_report_serialises_with_none_for_nan():
    import json
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd.utils.metrics import error_report_json
    plain = error_report_json(utils.KeypointErrorAnalyzer(2, conf_bins=4, conf_thresholds=[0.5]).compute())
    back = json.loads(json.dumps(plain))
    assert back["joints"][1]["mean"] is None and back["joints"][1]["quantiles"] == [None] * 5 and back["calibration"]["count"] == [0] * 4
    assert back["pr"]["thresholds"] == [0.5] and back["n"] == 0


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_fixed_order_sum_is_a_sum_and_skips_nan():
    g = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 1000):
        row = np.abs(g.standard_normal(n)).astype(F32)
        row[::7] = np.nan
        want = np.nansum(row.astype(F64))
        assert abs(enp.fixed_order_sum(row) - want) <= (n + 16) * 2.0 ** -52 * want
    ints = np.arange(1000, dtype=F32)                             # exact in any order
    assert enp.fixed_order_sum(ints) == 499500.0
    s = enp.summary(np.array([np.nan, 2.0, 0.5, np.nan], F32))
    assert s.tolist() == [2.0, 2.5, 0.5, 2.0] and enp.summary(np.full(4, np.nan, F32)).tolist() == [0.0] * 4


def test_hand_made_pairs_of_the_shared_case():
    pred, gt, vis, norm, conf, edges, thr = enp.error_case(257, 17, True, True)
    err = enp.errors(pred, gt, vis, norm)
    assert err[0, 0] == 0.0 and err[1, 0] == enp.PIXEL_THR and not (err[1, 0] < enp.PIXEL_THR)
    assert conf[0, 0] == edges[3] and conf[1, 0] == edges[-1] == 1.0 and conf[2, 0] == thr[37]
    count, hit = enp.calibration(err[:1, :1], conf[:1, :1], enp.PIXEL_THR, edges)
    assert count[0].tolist() == [0, 0, 0, 1] + [0] * 6 and hit[0].tolist() == count[0].tolist()       # ON the edge: the upper bin
    assert enp.calibration(err[1:2, :1], conf[1:2, :1], enp.PIXEL_THR, edges)[0].sum() == 0                  # ON the last edge: dropped
    assert enp.pr_hist(err[2:3, :1], conf[2:3, :1], enp.PIXEL_THR, thr)[0, 0, 37] == 1                       # ON threshold 37: not above it
    assert np.isnan(err).any() and np.isnan(conf).any() and (norm <= 0).any() and np.isinf(pred).any()


# ------------------------------------------------------------------------------------------------ validate.py
def test_validate_parser_accepts_the_two_flags():
    import validate as V
    p = V.build_parser()
    args = p.parse_args(["--checkpoint", "x.pth"])
    assert args.error_report is None and args.error_px == 10.0
    args = p.parse_args(["--checkpoint", "x.pth", "--error_report", "report.json", "--error_px", "5"])
    assert args.error_report == "report.json" and args.error_px == 5.0
