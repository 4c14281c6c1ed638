"""Pose rescoring and OKS-NMS on the device (pk_pose_rescore / pk_oks_nms) against the independent numpy restatement (tests/oks_nms_np.py),
and validate() on detector boxes end to end.

keep, n_keep and order must equal the restatement's EXACTLY.  That is a fair demand only where no decision hangs on the last bits (the
device's exp may differ from numpy's by an ulp), so every seeded case first asserts the restatement's margin >= 1e-9 (hard mode: the
nearest |oks - thr|; soft mode: the nearest relative gap between the two best current scores), and, so that the data exercises the
chain, that in every image of 20 and more poses hard NMS at the case's threshold removes at least 10 % and keeps at least 50 %.  These are
conditions on the generator's data, asserted, never skipped; the seeds below were chosen on the CPU with exactly this generator.
Tolerances: rescore relative 1e-13 (K sequential fp64 adds and one divide: K ulp at most, 64 x 1.1e-16 = 7e-15); soft out_score relative
1e-12 for max_dets <= 64 (each decay factor exp(-oks^2 / thr) carries the few-ulp error of oks scaled by 2 oks^2 / thr <= 2.3, and at most
64 factors multiply)."""
import functools
import json
import logging
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oks_nms_np as onp  # noqa: E402

pytestmark = pytest.mark.gpu

# empty images first, in the middle and last; 65 crosses a wave, 257 a 256-thread group
COUNTS = (0, 1, 2, 3, 0, 20, 65, 257, 0)
KS = (1, 13, 17, 64)
# per K the first seed whose data meets the conditions above for every (thr, in_vis_thr) of its cases (searched on the CPU, from 0 up)
HARD_SEED = {1: 0, 13: 0, 17: 1, 64: 0}
SOFT_SEED = {1: 0, 13: 0, 17: 0, 64: 0}
NEG_INF = -math.inf
VARS17 = (2.0 * onp.COCO_SIGMAS) ** 2


@functools.lru_cache(maxsize=None)
def _data(counts, K, seed, tie):
    return onp.make_batch(counts, K, seed, tie)


@functools.lru_cache(maxsize=None)
def _want(counts, K, seed, tie, thr, in_vis_thr, soft, max_dets):
    """The restatement's result, computed once per case and shared (never modified)."""
    kpt, area, score, off, vars_ = _data(counts, K, seed, tie)
    return onp.oks_nms_np(kpt, area, score, off, vars_, thr, in_vis_thr, soft, max_dets)


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _run(data, thr, in_vis_thr, soft, max_dets):
    from infantposeestimation_gaussianbias_amd import hipops
    kpt, area, score, off, vars_ = data
    out = hipops.oks_nms(_dev(kpt), _dev(area), _dev(score), off, _dev(vars_), thr, in_vis_thr, soft, max_dets)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _assert_conditions(counts, K, seed, tie, thr, in_vis_thr, margin):
    assert margin >= 1e-9, f"margin {margin:.3e}: the data sits on a decision; choose another seed"
    _, n_keep, _, _, hard_margin = _want(counts, K, seed, tie, thr, in_vis_thr, False, 0)
    for n, k in zip(counts, n_keep.tolist()):
        if n >= 20:
            assert n - k >= 0.1 * n and k >= 0.5 * n, f"{n} poses, {k} kept: the data does not exercise the chain"
    return hard_margin


def _check(counts, K, seed, thr, in_vis_thr, soft, max_dets):
    tie = not soft                                   # one tied score pair per image in hard mode, none in soft mode
    data = _data(counts, K, seed, tie)
    keep_w, nk_w, order_w, score_w, margin = _want(counts, K, seed, tie, thr, in_vis_thr, soft, max_dets)
    _assert_conditions(counts, K, seed, tie, thr, in_vis_thr, margin)
    keep, n_keep, order, out_score = _run(data, thr, in_vis_thr, soft, max_dets)
    assert keep.dtype == np.uint8 and n_keep.dtype == np.int32 and order.dtype == np.int32 and out_score.dtype == np.float64
    assert np.array_equal(n_keep, nk_w)
    assert np.array_equal(keep, keep_w)
    assert np.array_equal(order, order_w)
    if soft:
        assert max_dets <= 64
        err = np.abs(out_score - score_w)
        print(f"soft out_score: max relative error {float((err / np.maximum(np.abs(score_w), 1e-300)).max()):.3e}")
        assert np.all(err <= 1e-12 * np.abs(score_w))
    else:
        assert np.array_equal(out_score, score_w)    # the input score of a kept pose, bit for bit; 0 elsewhere
    # two launches on the same data: identical bytes
    again = _run(data, thr, in_vis_thr, soft, max_dets)
    for a, b in zip((keep, n_keep, order, out_score), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("in_vis_thr", [0.2, NEG_INF])
@pytest.mark.parametrize("thr", [0.9, 0.5])
@pytest.mark.parametrize("K", KS)
def test_hard_nms_matches_the_restatement(K, thr, in_vis_thr):
    _check(COUNTS, K, HARD_SEED[K], thr, in_vis_thr, False, 0)


@pytest.mark.parametrize("max_dets,thr,in_vis_thr", [(1, 0.9, 0.2), (20, 0.5, 0.2), (20, 0.9, NEG_INF), (64, 0.5, NEG_INF), (64, 0.9, 0.2)])
@pytest.mark.parametrize("K", KS)
def test_soft_nms_matches_the_restatement(K, max_dets, thr, in_vis_thr):
    """max_dets 1 and 20 cut the larger images short; 64 is above n for the images of 1, 2, 3 and 20 poses (selection until none remains)."""
    _check(COUNTS, K, SOFT_SEED[K], thr, in_vis_thr, True, max_dets)


@pytest.mark.parametrize("n,K,thr,in_vis_thr,soft,max_dets", [
    (20, 17, 0.9, 0.2, False, 0), (20, 17, 0.5, 0.2, True, 20),
    (1024, 17, 0.9, 0.2, False, 0), (1024, 64, 0.5, NEG_INF, False, 0),
    (1024, 13, 0.5, 0.2, True, 20), (1024, 64, 0.9, NEG_INF, True, 64)])
def test_one_image(n, K, thr, in_vis_thr, soft, max_dets):
    """n_img = 1, up to the 1024 poses one workgroup holds."""
    _check((n,), K, 300 + K + n, thr, in_vis_thr, soft, max_dets)


def test_more_than_1024_poses_in_an_image_raises():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    n = 1025
    z = lambda *s: torch.ones(*s, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PoseKernelError, match=r"image 1 holds 1025 poses"):
        hipops.oks_nms(z(n + 3, 17, 3), z(n + 3), z(n + 3), np.array([0, 3, n + 3], np.int32), z(17), 0.9)
    assert hipops.OKS_NMS_MAX_POSES == 1024


@pytest.mark.parametrize("soft", [False, True])
def test_nan_scores_go_last(soft):
    counts, K, seed, thr = (3, 20, 65), 17, 5, 0.9
    kpt, area, score, off, vars_ = onp.make_batch(counts, K, seed, tie=False)
    score = score.copy()
    score[[0, 3 + 7, 23 + 64]] = math.nan             # one per image; in the last image the last pose
    want = onp.oks_nms_np(kpt, area, score, off, vars_, thr, 0.2, soft, 64)
    assert want[4] >= 1e-9
    keep, n_keep, order, out_score = _run((kpt, area, score, off, vars_), thr, 0.2, soft, 64)
    assert np.array_equal(keep, want[0]) and np.array_equal(n_keep, want[1]) and np.array_equal(order, want[2])
    for i, p in enumerate((0, 7, 64)):                # where the NaN pose is kept, it is the image's last selection
        if keep[off[i] + p]:
            assert order[off[i] + n_keep[i] - 1] == p and math.isnan(out_score[off[i] + p])
    ok = ~np.isnan(want[3])
    assert np.array_equal(np.isnan(out_score), ~ok) and np.all(np.abs(out_score[ok] - want[3][ok]) <= 1e-12 * np.abs(want[3][ok]))


@pytest.mark.parametrize("K", KS)
def test_rescore_matches_the_restatement(K):
    from infantposeestimation_gaussianbias_amd import hipops
    rng = np.random.default_rng(K)
    n = 257
    kpt = rng.uniform(0, 1, (n, K, 3))
    kpt[3, :, 2] = 0.1                                  # nothing above 0.2: score 0
    kpt[4, :, 2] = 0.2                                  # the comparison is strict
    box = rng.uniform(0.05, 1, n)
    for thr in (0.2, NEG_INF):
        for b in (box, None):
            want = onp.rescore_np(kpt, b, thr)
            got = hipops.pose_rescore(_dev(kpt), None if b is None else _dev(b), thr).cpu().numpy()
            err = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
            print(f"rescore K={K} thr={thr}: max relative error {err:.3e}")
            assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want))
            if thr == 0.2:
                assert got[3] == 0.0 and got[4] == 0.0
    assert hipops.pose_rescore(_dev(kpt[:0]), None).shape == (0,)


def test_public_functions_return_kept_indices_and_scores():
    from infantposeestimation_gaussianbias_amd.utils import oks_nms, soft_oks_nms
    counts, K, seed = (0, 3, 20, 0, 65), 17, 117
    kpt, area, score, off, vars_ = _data(counts, K, seed, True)
    keep_w, nk_w, order_w, _, margin = _want(counts, K, seed, True, 0.9, 0.2, False, 0)
    assert margin >= 1e-9
    want_idx = np.concatenate([off[i] + order_w[off[i]:off[i] + nk_w[i]] for i in range(len(counts))])
    got = oks_nms(kpt, score, area, thr=0.9, offsets=off)                       # numpy in, numpy out; the default sigmas are COCO's
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want_idx)
    got_t = oks_nms(_dev(kpt), _dev(score), _dev(area), thr=0.9, sigmas=onp.COCO_SIGMAS, offsets=torch.from_numpy(off))
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want_idx)
    # one image, soft
    k1, a1, s1, _, _ = _data((20,), K, seed + 1, False)
    w = onp.oks_nms_np(k1, a1, s1, np.array([0, 20], np.int32), vars_, 0.5, 0.2, True, 5)
    assert w[4] >= 1e-9
    idx, sc = soft_oks_nms(k1, s1, a1, thr=0.5, max_dets=5)
    assert np.array_equal(idx, w[2][:5]) and np.all(np.abs(sc - w[3][idx]) <= 1e-12 * w[3][idx])
    assert oks_nms(kpt[:0], score[:0], area[:0]).shape == (0,)


# ------------------------------------------------------------------------------------------------ validate() on detector boxes
def _tiny_set(root, n_img=3):
    """Three PNG images with two annotated people each, and a detection file: per image two IDENTICAL boxes with different scores and one
    distant box."""
    import coco_cases as cc
    from PIL import Image
    rng = np.random.default_rng(0)
    os.makedirs(root / "val", exist_ok=True)
    images, anns, dets, aid = [], [], [], 1
    for i in range(n_img):
        H, W = 160 + 20 * i, 140 + 10 * i
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "val" / f"{i}.png")
        images.append({"id": 100 + i, "file_name": f"{i}.png", "width": W, "height": H})
        for j in range(2):
            kp = cc.pose(17, 20 + 50 * j, 30, 60, rng)
            anns.append(cc.gt_ann(aid, 100 + i, kp, 60 * 60 * 0.8 + 3000 * j, bbox=[15 + 50 * j, 25, 70, 70]))
            aid += 1
        dets += [{"image_id": 100 + i, "category_id": 1, "bbox": [15, 25, 70, 70], "score": 0.6 + 0.1 * i},
                 {"image_id": 100 + i, "category_id": 1, "bbox": [65, 25 + 60 + 10 * i, 60, 60], "score": 0.5},
                 {"image_id": 100 + i, "category_id": 1, "bbox": [15, 25, 70, 70], "score": 0.95 - 0.1 * i}]
    ann = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}
    (root / "ann.json").write_text(json.dumps(ann))
    (root / "dets.json").write_text(json.dumps(dets))
    return dets


def _cfg(root, **kw):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    cfg = get_config("hrnet_w18")
    cfg.data.data_root, cfg.data.val_ann, cfg.data.val_img_prefix = str(root), "ann.json", "val/"
    cfg.train.batch_size, cfg.train.num_workers = 2, 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _restate_kept(preds, thr, in_vis_thr, soft):
    """The restatement applied to the evaluator's records -> [(record index, score)] in the evaluator's order."""
    from infantposeestimation_gaussianbias_amd.utils import COCOEvaluator
    ids = list(dict.fromkeys(r["image_id"] for r in preds))
    idx = [i for img in ids for i, r in enumerate(preds) if r["image_id"] == img]
    off = np.concatenate([[0], np.cumsum([sum(r["image_id"] == img for r in preds) for img in ids])]).astype(np.int32)
    kpt = np.array([preds[i]["keypoints"] for i in idx]).reshape(len(idx), 17, 3)
    score = onp.rescore_np(kpt, np.array([preds[i]["box_score"] for i in idx]), in_vis_thr)
    area = np.array([preds[i]["area"] for i in idx])
    _, n_keep, order, out, margin = onp.oks_nms_np(kpt, area, score, off, (2 * COCOEvaluator.DEFAULT_OKS_SIGMAS) ** 2, thr, in_vis_thr, soft, 20)
    return [(idx[off[i] + p], out[off[i] + p]) for i in range(len(ids)) for p in order[off[i]:off[i] + n_keep[i]]], margin


@pytest.mark.parametrize("soft", [False, True])
def test_validate_on_detector_boxes(tmp_path, soft):
    import validate as V
    from infantposeestimation_gaussianbias_amd.datasets import build_dataloader
    from infantposeestimation_gaussianbias_amd.models import build_model
    from infantposeestimation_gaussianbias_amd.utils import COCOEvaluator
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import STAT_KEYS, COCOKeypointEval
    dets = _tiny_set(tmp_path)
    # in_vis_thr -inf: an untrained network's heatmap maxima are small, and every joint must count for the duplicates' OKS to be exactly 1
    cfg = _cfg(tmp_path, bbox_file="dets.json", oks_nms_thr=0.9, in_vis_thr=NEG_INF, soft_nms=soft)
    torch.manual_seed(0)
    model = build_model(cfg).cuda()
    log, dev = logging.getLogger("test"), torch.device("cuda")
    ann = str(tmp_path / "ann.json")
    ev = COCOEvaluator(ann_file=ann, num_keypoints=17, oks_nms_thr=0.9, in_vis_thr=NEG_INF, soft_nms=soft)
    metrics, preds = V.validate(model, build_dataloader(cfg, is_train=False), dev, cfg, log, flip_test=True, evaluator=ev)
    assert set(metrics) == set(STAT_KEYS) | {"loss"} and math.isnan(metrics["loss"])
    assert preds is ev.predictions and len(ev.predictions) == len(dets) == 9
    assert [r["box_score"] for r in preds] == [d["score"] for d in dets] and all(r["ann_id"] == -1 for r in preds)
    # identical boxes -> identical crops -> the same pose twice (to the last bits where both crops went through the same kernels): OKS 1
    for i in range(3):
        a, b = (np.array(preds[j]["keypoints"]).reshape(17, 3) for j in (3 * i, 3 * i + 2))
        assert onp.oks_to(a, preds[3 * i]["area"], b[None], np.array([preds[3 * i + 2]["area"]]), VARS17, NEG_INF)[0] > 1 - 1e-6
    want, margin = _restate_kept(preds, 0.9, NEG_INF, soft)
    assert margin >= 1e-9
    assert [preds.index(next(p for p in preds if p["image_id"] == k["image_id"] and p["keypoints"] == k["keypoints"]
                             and p["box_score"] == k["box_score"])) for k in ev.kept] == [i for i, _ in want]
    for k, (i, s) in zip(ev.kept, want):
        assert abs(k["score"] - s) <= 1e-12 * abs(s)
        assert {kk: v for kk, v in k.items() if kk != "score"} == {kk: v for kk, v in preds[i].items() if kk != "score"}
    kept_idx = [i for i, _ in want]
    if not soft:
        # of the two identical poses of an image (records 3 i and 3 i + 2) the lower-scored one is gone.  Scores are the rescored ones: box
        # score x mean keypoint score, so the higher box score wins unless the untrained network's mean keypoint score is negative
        rescored = onp.rescore_np(np.array([r["keypoints"] for r in preds]).reshape(9, 17, 3), np.array([r["box_score"] for r in preds]), NEG_INF)
        for i in range(3):
            a, b = 3 * i, 3 * i + 2
            winner, loser = (a, b) if rescored[a] >= rescored[b] else (b, a)
            assert winner in kept_idx and loser not in kept_idx
        assert len(ev.kept) <= 6
    else:               # soft: nothing is removed below max_dets, the duplicates only decay
        assert len(ev.kept) == 9
    # the metrics are those of the surviving records, and the evaluator's own records are untouched
    direct = COCOKeypointEval(ann, COCOEvaluator.DEFAULT_OKS_SIGMAS).evaluate(ev.kept)
    for key in STAT_KEYS:
        assert metrics[key] == direct[key], key
    # the same loader without an NMS threshold evaluates all boxes
    cfg_all = _cfg(tmp_path, bbox_file="dets.json")
    m_all, p_all = V.validate(model, build_dataloader(cfg_all, is_train=False), dev, cfg_all, log, flip_test=True)
    assert len(p_all) == 9 and math.isnan(m_all["loss"])
    direct = COCOKeypointEval(ann, COCOEvaluator.DEFAULT_OKS_SIGMAS).evaluate(p_all)
    for key in STAT_KEYS:
        assert m_all[key] == direct[key], key
    if not soft:
        # PCK needs ground truth
        with pytest.raises(RuntimeError, match="PCK"):
            V.validate(model, build_dataloader(cfg_all, is_train=False), dev, cfg_all, log, flip_test=False, pck_thresholds=(0.2,))
        # ground-truth boxes: evaluate() with oks_nms_thr=None is COCOKeypointEval over the predictions, as before
        cfg_gt = _cfg(tmp_path)
        ev_gt = COCOEvaluator(ann_file=ann, num_keypoints=17)
        m_gt, p_gt = V.validate(model, build_dataloader(cfg_gt, is_train=False), dev, cfg_gt, log, flip_test=True, evaluator=ev_gt)
        assert len(p_gt) == 6 and not math.isnan(m_gt["loss"]) and ev_gt.kept == [] and all("box_score" not in r for r in p_gt)
        direct = COCOKeypointEval(ann, COCOEvaluator.DEFAULT_OKS_SIGMAS).evaluate(p_gt)
        for key in STAT_KEYS:
            assert m_gt[key] == direct[key], key
