"""Localisation error analysis on the device: pk_kpt_error and pk_kpt_error_quantiles against their numpy restatements
(tests/error_analysis_np.py) at the sizes where the kernels change behaviour (one sample, the 256-thread boundary, a wrapped stride with a
ragged tail, a row stride beyond the batch), `KeypointErrorAnalyzer` over a store that grows, and validate(error_analysis=).

No tolerance anywhere.  Every output is an integer count, an order statistic or a float64 sum taken in a fixed order that the restatement
repeats; the error itself is float32 arithmetic with one rounding per operation.  Bits are compared, and two launches must give the same."""
import functools
import json
import logging

import numpy as np
import pytest
import torch

import error_analysis_np as enp

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = np.float32, np.float64
SENTINEL = 3.0e38                                                 # fills what a launch must leave alone


def G(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV, dtype)      # a copy: the cached cases are read-only


def same_bits(a, b):
    """float arrays equal bit for bit, all NaNs alike (the store's NaN marks 'not counted')."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0, a).view(np.uint8), np.where(np.isnan(b), 0, b).view(np.uint8))


# ------------------------------------------------------------------------------------------------ pk_kpt_error
@functools.lru_cache(maxsize=None)
def _want(N, K, with_norm, with_conf):
    pred, gt, vis, norm, conf, edges, thr = enp.error_case(N, K, with_norm, with_conf)
    err = enp.errors(pred, gt, vis, norm)
    if not with_conf:
        return err, None
    return err, enp.calibration(err, conf, enp.PIXEL_THR, edges) + (enp.pr_hist(err, conf, enp.PIXEL_THR, thr),)


def _device(case, pad, parts=1):
    """The case through hipops in `parts` updates -> store (K, N + pad) and the three counters (or None)."""
    from infantposeestimation_gaussianbias_amd import hipops
    pred, gt, vis, norm, conf, edges, thr = case
    N, K = vis.shape
    store = torch.full((K, N + pad), SENTINEL, device=DEV)
    buf = hipops.kpt_error_buffers(K, len(edges) - 1, len(thr), DEV) if conf is not None else None
    de, dt = G(edges), G(thr)
    for idx in np.array_split(np.arange(N), parts):
        if conf is None:
            hipops.kpt_error_accumulate(G(pred[idx]), G(gt[idx]), G(vis[idx]), store, int(idx[0]), float(enp.PIXEL_THR),
                                        normalizer=None if norm is None else G(norm[idx]))
        else:
            hipops.kpt_error_accumulate(G(pred[idx]), G(gt[idx]), G(vis[idx]), store, int(idx[0]), float(enp.PIXEL_THR), G(conf[idx]),
                                        None if norm is None else G(norm[idx]), de, dt, *buf)
    return store, buf


@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_errors_and_counters_equal_the_restatement(N):
    seen = 0
    for K in (1, 17):
        for with_norm in (False, True):
            for with_conf in (False, True):
                case = enp.error_case(N, K, with_norm, with_conf)
                err, counters = _want(N, K, with_norm, with_conf)
                for pad in (0, 3):                                # ld = N and ld = N + 3
                    tag = (K, with_norm, with_conf, pad)
                    store, buf = _device(case, pad)
                    again, buf2 = _device(case, pad)
                    assert torch.equal(store.view(torch.int32), again.view(torch.int32)), ("two launches differ in their bits", tag)
                    got = store.cpu().numpy()
                    assert same_bits(got[:, :N], np.ascontiguousarray(err.T)), tag
                    assert (got[:, N:] == F32(SENTINEL)).all(), ("wrote beyond its N columns", tag)
                    if with_conf:
                        assert all(torch.equal(a, b) for a, b in zip(buf, buf2)), tag
                        for name, g_, w in zip(("calib_count", "calib_hit", "pr_hist"), buf, counters):
                            assert g_.dtype == torch.int64 and np.array_equal(g_.cpu().numpy(), w), (name, tag)
                    if N > 1:                                     # two updates over a split batch: the same store, the same counters
                        split, sbuf = _device(case, pad, parts=2)
                        assert torch.equal(split.view(torch.int32), store.view(torch.int32)), tag
                        assert not with_conf or all(torch.equal(a, b) for a, b in zip(buf, sbuf)), tag
                if with_conf:
                    seen += int(counters[2].sum())
                    conf = case[4]
                    used = ~np.isnan(err) & np.isfinite(conf)
                    assert counters[2].sum() == used.sum() and counters[0].sum() <= used.sum()
                    assert N < 200 or (counters[0].sum() < used.sum() < (~np.isnan(err)).sum() < err.size)
                    assert np.array_equal(counters[0].sum(1) >= counters[1].sum(1), np.ones(K, bool))
    print(f"N={N}: store bits and counters equal; {seen} pairs entered precision / recall")


def test_the_hand_made_pairs_on_the_device():
    """pred == gt is error 0 and a hit; an error exactly equal to the threshold is not; a confidence on an inner edge counts in the upper
    bin, on the last edge (1.0, the reference's) in none, on a threshold not above it."""
    pred, gt, vis, norm, conf, edges, thr = case = enp.error_case(6, 1, False, True)
    store, (count, hit, hist) = _device(case, 0)
    e = store.cpu().numpy()[0]
    assert e[0] == 0.0 and e[1] == 10.0 and e[3] == 3.0 and e[4] == 0.5
    count, hit, hist = count.cpu().numpy()[0], hit.cpu().numpy()[0], hist.cpu().numpy()[0]
    # confidences: edges[3], 1.0 (dropped), thr[37] = 37/99 (bin 3), 1.0 (dropped), edges[0] = 0 (bin 0), thr[0] = 0 (bin 0); errors
    # 0, 10 (miss), sqrt 5, 3, 0.5, sqrt 100 = 10 (miss)
    assert count.tolist() == [2, 0, 0, 2] + [0] * 6 and hit.tolist() == [1, 0, 0, 2] + [0] * 6
    want = np.zeros((2, 101), np.int64)
    for c, miss in ((edges[3], 0), (1.0, 1), (thr[37], 0), (1.0, 0), (0.0, 0), (0.0, 1)):
        want[miss, int((F32(c) > thr).sum())] += 1
    assert np.array_equal(hist, want) and hist[0, 37] == 1 and hist[:, 0].tolist() == [1, 1] and hist[:, 99].tolist() == [1, 1]


def test_empty_batch_launches_nothing():
    from infantposeestimation_gaussianbias_amd import hipops
    z = torch.zeros
    store = torch.full((3, 4), SENTINEL, device=DEV)
    buf = hipops.kpt_error_buffers(3, 10, 100, DEV)
    hipops.kpt_error_accumulate(z(0, 3, 2, device=DEV), z(0, 3, 2, device=DEV), z(0, 3, device=DEV), store, 4, 10.0, z(0, 3, device=DEV), None,
                                z(11, device=DEV), z(100, device=DEV), *buf)
    assert (store == SENTINEL).all() and not any(b.any() for b in buf)
    order, summary = hipops.kpt_error_quantiles(store, 0, z(2, dtype=torch.float64, device=DEV))
    assert tuple(order.shape) == (3, 2, 2) and not order.any() and not summary.any()


# ------------------------------------------------------------------------------------------------ pk_kpt_error_quantiles
@pytest.mark.parametrize("n_cols", [1, 2, 255, 256, 257, 1000])
def test_order_statistics_and_summary_equal_the_restatement(n_cols):
    from infantposeestimation_gaussianbias_amd import hipops
    q = enp.QUANTILES
    whole = part = tied = 0
    for pad in (0, 3):
        host = enp.store_case(n_cols, n_cols + pad)
        store = G(host)
        order_t, summary_t = hipops.kpt_error_quantiles(store, n_cols, G(q, torch.float64))
        again = hipops.kpt_error_quantiles(store, n_cols, G(q, torch.float64))
        assert torch.equal(order_t.view(torch.int32), again[0].view(torch.int32)) and torch.equal(summary_t.view(torch.int64), again[1].view(torch.int64))
        order, summary = order_t.cpu().numpy(), summary_t.cpu().numpy()
        assert order.shape == (5, len(q), 2) and order.dtype == F32 and summary.shape == (5, 4) and summary.dtype == F64
        for k, kind in enumerate(enp.ROW_KINDS):
            row = host[k, :n_cols]
            want_o, want_s = enp.order_stats(row, q), enp.summary(row)
            assert np.array_equal(order[k].view(np.uint32), want_o.view(np.uint32)), (kind, pad, order[k], want_o)
            assert np.array_equal(summary[k].view(np.uint64), want_s.view(np.uint64)), (kind, pad, summary[k], want_s)
            n = int(want_s[0])
            for qj, (lo_v, hi_v) in zip(q, want_o):
                pos = qj * (n - 1) if n else 0.0
                whole, part = whole + (n > 1 and pos == np.floor(pos)), part + (pos != np.floor(pos))
                tied += n > 1 and pos != np.floor(pos) and lo_v == hi_v
        assert summary[0].tolist() == [0.0] * 4 and not order[0].any() and summary[1].tolist() == [1.0, 2.5, 2.5, 2.5]
        assert (order[1] == 2.5).all()
        if n_cols > 3:
            assert np.isinf(order[3, 1]).all() and order[3, 0, 0] == 0.0 and summary[3, 3] == np.inf and summary[3, 1] == np.inf
    assert n_cols < 255 or (whole and part and tied), (whole, part, tied)
    print(f"n_cols={n_cols}: order statistics and summary equal bit for bit; positions: {whole} whole, {part} fractional, {tied} of those between ties")


def test_quantiles_beyond_the_unit_interval_stay_inside_the_row():
    """q is device data the entry cannot check: a value outside [0, 1] or NaN is clamped to an end, never read past the row."""
    from infantposeestimation_gaussianbias_amd import hipops
    host = enp.store_case(257, 260)
    order = hipops.kpt_error_quantiles(G(host), 257, G(np.array([-0.5, 1.5, np.nan]), torch.float64))[0].cpu().numpy()
    v = np.sort(host[4, :257])
    assert order[4].tolist() == [[v[0], v[1]], [v[-1], v[-1]], [v[0], v[1]]]


# ------------------------------------------------------------------------------------------------ KeypointErrorAnalyzer
def _batches(K=17, sizes=(100, 100, 100)):
    pred, gt, vis, norm, conf, edges, thr = enp.error_case(sum(sizes), K, False, True, seed=3)
    cuts = np.cumsum((0,) + tuple(sizes))
    return tuple(np.array(a) for a in (pred, gt, vis, conf)), [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]      # writable copies


def _fill(analyzer, arrays, slices, to=lambda a: a):
    for s in slices:
        analyzer.update(*(to(a[s]) for a in arrays))
    return analyzer.compute()


def test_analyzer_quantiles_equal_numpy_percentile_over_a_store_that_grows():
    from infantposeestimation_gaussianbias_amd import utils
    arrays, slices = _batches()
    a = utils.KeypointErrorAnalyzer(17, capacity=256)
    caps = []
    for s in slices:
        a.update(*(x[s] for x in arrays))
        caps.append(int(a._store.shape[1]))
    assert caps == [256, 256, 512], "three batches of 100 force exactly one growth of a store of 256"
    res = a.compute()
    err = enp.errors(*arrays[:3])
    for k, joint in enumerate(res["joints"]):
        v = err[:, k][~np.isnan(err[:, k])].astype(F64)
        assert joint["n"] == len(v) > 0
        assert np.array_equal(joint["quantiles"], np.quantile(v, a.quantiles)), k
        assert np.array_equal(joint["quantiles"], np.percentile(v, [5, 25, 50, 75, 95])), k
        assert joint["min"] == v.min() and joint["max"] == v.max() and joint["mean"] == enp.fixed_order_sum(err[:, k]) / len(v)
    assert res["n"] == (~np.isnan(err)).sum()


def test_analyzer_curves_equal_the_reference_loops_and_numpy_input_equals_device_input():
    from infantposeestimation_gaussianbias_amd import utils
    arrays, slices = _batches()
    pred, gt, vis, conf = arrays
    make = lambda: utils.KeypointErrorAnalyzer(17, conf_bins=enp.REFERENCE_EDGES, capacity=64)
    res = _fill(make(), arrays, slices)
    err = enp.errors(pred, gt, vis)
    count, hit = enp.calibration(err, conf, 10.0, enp.REFERENCE_EDGES)
    tp, fp, fn = enp.pr_reference(err, conf, 10.0, enp.REFERENCE_THRESHOLDS)
    centre = (enp.REFERENCE_EDGES.astype(F32).astype(F64)[:-1] + enp.REFERENCE_EDGES.astype(F32).astype(F64)[1:]) / 2

    def check(got_cal, got_pr, count, hit, tp, fp, fn):
        accuracy = np.array([h / c if c > 0 else 0 for h, c in zip(hit.tolist(), count.tolist())], F64)      # the reference's mean, or 0
        assert np.array_equal(got_cal["count"], count) and np.array_equal(got_cal["accuracy"], accuracy)
        assert got_cal["ece"] == (count * np.abs(accuracy - centre)).sum() / count.sum()
        precision, recall, area = enp.reference_curves(tp, fp, fn)
        assert np.array_equal(got_pr["precision"], precision) and np.array_equal(got_pr["recall"], recall)
        assert got_pr["ap"] == -area and area < 0, "the reference integrates over a falling recall: negative; ours is its negation"

    for k, joint in enumerate(res["joints"]):
        check(joint["calibration"], joint["pr"], count[k], hit[k], tp[k], fp[k], fn[k])
    check(res["calibration"], res["pr"], count.sum(0), hit.sum(0), tp.sum(0), fp.sum(0), fn.sum(0))
    assert res["ece"] == res["calibration"]["ece"] and res["ap"] == res["pr"]["ap"]
    # the default edges keep the pairs with a confidence of exactly 1.0, which the reference's edges drop
    dflt = _fill(utils.KeypointErrorAnalyzer(17), arrays, slices)
    ones = (~np.isnan(err) & (conf == 1.0)).sum()
    assert ones >= 2 and dflt["calibration"]["count"].sum() == count.sum() + ones and dflt["calibration"]["count"][-1] == count.sum(0)[-1] + ones
    # device tensors in: the same report, array by array
    dev = _fill(make(), arrays, slices, to=G)

    def flat(r):
        out = [r["quantiles"], np.array([r["n"], r["ece"], r["ap"]])]
        for part in [r] + r["joints"]:
            out += [part["calibration"][k] for k in ("edges", "count", "accuracy")] + [part["pr"][k] for k in ("thresholds", "precision", "recall")]
            out += [np.array([part["calibration"]["ece"], part["pr"]["ap"]])]
        for j in r["joints"]:
            out += [j["quantiles"], np.array([j["n"], j["mean"], j["min"], j["max"]])]
        return out

    assert all(same_bits(a, b) for a, b in zip(flat(res), flat(dev))) and len(flat(res)) == len(flat(dev))
    # the one-shot form, and a batch without confidences: it enters the distribution only
    once = utils.keypoint_error_report(pred, gt, vis, conf, conf_bins=enp.REFERENCE_EDGES)
    assert all(same_bits(a, b) for a, b in zip(flat(res), flat(once)))
    a = make()
    a.update(pred[:100], gt[:100], vis[:100], conf[:100])
    a.update(pred[100:], gt[100:], vis[100:])
    mixed = a.compute()
    assert mixed["n"] == res["n"] and np.array_equal(mixed["joints"][3]["quantiles"], res["joints"][3]["quantiles"])
    assert np.array_equal(mixed["calibration"]["count"], enp.calibration(err[:100], conf[:100], 10.0, enp.REFERENCE_EDGES)[0].sum(0))


def test_analyzer_with_a_normalizer_reports_normalised_errors():
    from infantposeestimation_gaussianbias_amd import utils
    pred, gt, vis, norm, conf = (np.array(a) for a in enp.error_case(257, 17, True, True)[:5])
    res = utils.keypoint_error_report(pred, gt, vis, conf, norm, pixel_threshold=10.0, quantiles=(0.5,))
    err = enp.errors(pred, gt, vis, norm)
    for k, joint in enumerate(res["joints"]):
        assert joint["quantiles"][0] == np.median(err[:, k][~np.isnan(err[:, k])].astype(F64))


# ------------------------------------------------------------------------------------------------ validate.py
@functools.lru_cache(maxsize=None)
def _model():
    import os
    from conftest import GOLDEN
    from recipe import synth_state_dict
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        keys = json.load(f)
    m = PoseEstimator("hrnet_w18", 17, False, "heatmap", True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(keys["hrnet_w18_heatmap"], 41).items()}, strict=True)
    return m.to(DEV).eval()


def test_validate_writes_the_report_next_to_the_unchanged_metrics(tmp_path):
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import SyntheticLoader
    from infantposeestimation_gaussianbias_amd.utils import KeypointErrorAnalyzer
    cfg = get_config("hrnet_w18")
    cfg.train.batch_size = 4
    log, dev = logging.getLogger("test"), torch.device(DEV)
    seen = []

    class Recording(KeypointErrorAnalyzer):
        def update(self, pred, gt, visible, confidence=None, normalizer=None):
            assert normalizer is None and all(torch.is_tensor(t) and t.is_cuda for t in (pred, gt, visible, confidence))
            seen.append(tuple(t.detach().cpu().numpy().copy() for t in (pred, gt, visible, confidence)))
            return super().update(pred, gt, visible, confidence, normalizer)

    plain, _ = V.validate(_model(), SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False)
    # edges wide enough for any finite score: every counted pair with a finite score lands in a calibration bin
    analyzer = Recording(17, pixel_threshold=10.0, conf_bins=[-3.0e38, 0.5, 3.0e38])
    path = tmp_path / "report.json"
    with_report, _ = V.validate(_model(), SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False, error_analysis=analyzer,
                                error_report=str(path))
    assert set(with_report) == set(plain)
    for k in plain:
        assert with_report[k] == plain[k] or (np.isnan(with_report[k]) and np.isnan(plain[k])), k
    assert len(seen) == 2 and all(s[0].shape == (4, 17, 2) and s[3].shape == (4, 17) for s in seen)
    pred, gt, vis, conf = (np.concatenate([s[i] for s in seen]) for i in range(4))
    err = enp.errors(pred, gt, vis)
    counted = int((~np.isnan(err)).sum())
    scored = int((~np.isnan(err) & np.isfinite(conf)).sum())
    with open(path) as f:
        report = json.load(f)
    assert 0 < counted == report["n"] == sum(j["n"] for j in report["joints"]) and scored == sum(report["calibration"]["count"])
    assert report["calibration"]["count"] == enp.calibration(err, conf, 10.0, [-3.0e38, 0.5, 3.0e38])[0].sum(0).tolist()
    tp, fp, fn = (c.sum(0) for c in enp.pr_reference(err, conf, 10.0, enp.REFERENCE_THRESHOLDS))
    precision, recall, area = enp.reference_curves(tp, fp, fn)
    assert report["pr"]["precision"] == precision.tolist() and report["pr"]["recall"] == recall.tolist() and report["ap"] == -area
    k = next(k for k, j in enumerate(report["joints"]) if j["n"])
    assert report["joints"][k]["quantiles"] == np.quantile(err[:, k][~np.isnan(err[:, k])].astype(F64), [0.05, 0.25, 0.5, 0.75, 0.95]).tolist()
    assert report["pixel_threshold"] == 10.0 and report["quantiles"] == [0.05, 0.25, 0.5, 0.75, 0.95]


def test_validate_refuses_the_analysis_on_detector_boxes():
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.utils import KeypointErrorAnalyzer
    cfg = get_config("hrnet_w18")

    class Boxes:
        """One batch that carries box scores, as the COCO loader built with a bbox_file yields them."""
        dataset = None

        def __iter__(self):
            z = torch.zeros
            yield {"img": z(1, 3, cfg.data.input_size[1], cfg.data.input_size[0]),
                   "meta": {"box_score": torch.ones(1), "center": z(1, 2), "scale": torch.ones(1, 2), "image_id": [1], "ann_id": [1],
                            "area": [1.0], "bbox": z(1, 4)}}

        def __len__(self):
            return 1

    with pytest.raises(RuntimeError, match="error analysis needs ground-truth keypoints"):
        V.validate(_model(), Boxes(), torch.device(DEV), cfg, logging.getLogger("test"), flip_test=False, error_analysis=KeypointErrorAnalyzer(17))
