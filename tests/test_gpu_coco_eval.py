"""COCO keypoint AP / AR on the device (COCOKeypointEval over pk_coco_kpt_oks / pk_coco_kpt_eval) against hand-derived results and the
independent numpy restatement of COCOeval (tests/cocoeval_np.py); the COCOEvaluator / validate() integration end to end."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_cases as cc  # noqa: E402
import cocoeval_np  # noqa: E402

pytestmark = pytest.mark.gpu


def _eval(ann, recs, sigmas=cc.COCO_SIGMAS):
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import COCOKeypointEval
    ev = COCOKeypointEval(ann, sigmas)
    return ev, ev.evaluate(recs)


def _close(got, want, tol=1e-12):
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_hand_cases(case):
    ann, recs, want = getattr(cc, f"case_{case}")()
    ev, stats = _eval(ann, recs)
    _close(stats, want)
    if case == "a":
        assert 0.70 < ev.ious[1][0, 0] < 0.75
    if case == "c":
        # 20 of 25 detections kept: the five lowest-scored (record 20..24, on g3) are not among the slots
        assert ev.slot_record.size == 20 and set(ev.slot_record.tolist()) == set(range(20))
        m, ig = ev.dt_match[0], ev.dt_ignore[0]               # area 'all', (T, 20) in per-image score order
        slot_of = {int(r): s for s, r in enumerate(ev.slot_record)}
        assert np.all(m[:, slot_of[0]] == 1) and np.all(ig[:, slot_of[0]])            # on the num_keypoints == 0 ground truth: ignored
        for r in (1, 2, 3):                                                           # three detections absorbed by the crowd
            assert np.all(m[:, slot_of[r]] == 2) and np.all(ig[:, slot_of[r]])
        assert np.all(m[:, slot_of[4]] == 0) and not ig[:, slot_of[4]].any()           # the TP


def test_equal_oks_goes_to_the_later_ground_truth():
    ann, recs = cc.case_d()
    ev, _ = _eval(ann, recs)
    assert ev.ious[5].tolist() == [[1.0, 1.0]]
    assert np.all(ev.dt_match == 1)


def test_box_distance_oks_without_visible_joints():
    ann, recs, want = cc.case_e()
    ev, _ = _eval(ann, recs)
    got = ev.ious[9][:, 0]
    assert got[0] == 1.0
    assert abs(got[1] - want[1]) <= 4 * np.spacing(want[1])


def _check_against_restatement(ann, recs, sigmas):
    assert not cc.near_threshold(ann, recs, sigmas), "generator produced an OKS within 1e-12 of a threshold"
    want, prec, rec, ious, evalImgs = cocoeval_np.cocoeval(ann, recs, sigmas)
    ev, got = _eval(ann, recs, sigmas)
    assert set(ev.ious) == {i for i, v in ious.items() if len(v)}
    for i, v in ev.ious.items():
        assert v.shape == ious[i].shape
        assert np.all(np.abs(v - ious[i]) <= 4 * np.spacing(np.maximum(np.abs(ious[i]), 1e-300))), i
    assert np.array_equal(ev.precision, prec)
    assert np.array_equal(ev.recall, rec)
    _close(got, want)
    # matches of every capped slot == the restatement's (area 'all', per-image score order)
    slot = 0
    for i, img in enumerate(ev.img_ids.tolist()):
        e = evalImgs[0][i]
        if e is None:
            continue
        n = len(e['dtRec'])
        assert ev.slot_record[slot:slot + n].tolist() == e['dtRec']
        assert np.array_equal(ev.dt_match[0][:, slot:slot + n], e['dtGt'])
        slot += n
    assert slot == ev.slot_record.size
    # bitwise reproducible
    ev2, got2 = _eval(ann, recs, sigmas)
    assert got2 == got and np.array_equal(ev2.precision.view(np.uint64), ev.precision.view(np.uint64))
    assert all(np.array_equal(ev2.ious[i].view(np.uint64), v.view(np.uint64)) for i, v in ev.ious.items())


@pytest.mark.parametrize("seed", [0, 1])
def test_random_sets_match_the_restatement_k17(seed):
    ann, recs, sig = cc.random_set(seed, n_img=300)
    _check_against_restatement(ann, recs, sig)


def test_random_set_matches_the_restatement_k13_custom_sigmas():
    sig = np.random.default_rng(9).uniform(0.02, 0.11, 13)
    ann, recs, sig = cc.random_set(5, n_img=200, K=13, sigmas=sig)
    _check_against_restatement(ann, recs, sig)


def test_perfect_predictions():
    ann, recs, sig = cc.random_set(7, n_img=120, crowded=False, perfect=True)
    _, stats = _eval(ann, recs, sig)
    want, _, _, _, _ = cocoeval_np.cocoeval(ann, recs, sig)
    _close(stats, want)
    areas = {'': (0, 1e10), '_M': (32 ** 2, 96 ** 2), '_L': (96 ** 2, 1e10)}
    for sfx, (lo, hi) in areas.items():
        held = any(lo <= a['area'] <= hi and not a.get('iscrowd') and a['num_keypoints'] > 0 for a in ann['annotations'])
        for k in ('AP', 'AR'):
            assert abs(stats[k + sfx] - (1.0 if held else -1.0)) <= 1e-12, (k + sfx, stats[k + sfx])


def test_cocoevaluator_uses_the_native_evaluator(tmp_path):
    from infantposeestimation_gaussianbias_amd.utils import COCOEvaluator
    ann, recs, sig = cc.random_set(3, n_img=40)
    path = tmp_path / "ann.json"
    path.write_text(json.dumps(ann))
    ev = COCOEvaluator(ann_file=str(path))
    ev.predictions = [dict(r, area=1.0, bbox=[0, 0, 1, 1]) for r in recs]
    want, _, _, _, _ = cocoeval_np.cocoeval(ann, recs, sig)
    _close(ev.evaluate(), want)


# ------------------------------------------------------------------------------------------------ validate() end to end
def _tiny_coco(root, n_img=3):
    from PIL import Image
    rng = np.random.default_rng(0)
    os.makedirs(root / "val", exist_ok=True)
    images, anns, aid = [], [], 1
    for i in range(n_img):
        H, W = 160 + 20 * i, 140 + 10 * i
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "val" / f"{i}.png")
        images.append({"id": 100 + i, "file_name": f"{i}.png", "width": W, "height": H})
        for j in range(2):
            kp = cc.pose(17, 20 + 50 * j, 30, 60, rng)
            anns.append(cc.gt_ann(aid, 100 + i, kp, 60 * 60 * 0.8 + 3000 * j, bbox=[15 + 50 * j, 25, 70, 70]))
            aid += 1
    ann = {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}
    (root / "ann.json").write_text(json.dumps(ann))
    return ann


def _small_cfg(root):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    cfg = get_config("hrnet_w18")
    cfg.data.data_root, cfg.data.val_ann, cfg.data.val_img_prefix = str(root), "ann.json", "val/"
    cfg.train.batch_size, cfg.train.num_workers = 2, 0
    return cfg


def test_validate_reports_coco_ap_from_the_loaders_annotation_file(tmp_path):
    import validate as V
    from infantposeestimation_gaussianbias_amd.datasets import build_dataloader
    from infantposeestimation_gaussianbias_amd.models import build_model
    from infantposeestimation_gaussianbias_amd.utils import COCOEvaluator
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import STAT_KEYS, COCOKeypointEval
    _tiny_coco(tmp_path)
    cfg = _small_cfg(tmp_path)
    torch.manual_seed(0)
    model = build_model(cfg).cuda()
    loader = build_dataloader(cfg, is_train=False)
    metrics, preds = V.validate(model, loader, torch.device("cuda"), cfg, logging.getLogger("test"), flip_test=True)
    assert set(metrics) == set(STAT_KEYS) | {"loss"}
    assert len(preds) == 6
    want = COCOKeypointEval(str(tmp_path / "ann.json"), COCOEvaluator.DEFAULT_OKS_SIGMAS).evaluate(preds)
    for k in STAT_KEYS:
        assert metrics[k] == want[k], k
    # a synthetic loader keeps the stand-in, also with a real annotation file under data_root
    from infantposeestimation_gaussianbias_amd.datasets import SyntheticLoader
    metrics, _ = V.validate(model, SyntheticLoader(cfg, n_batches=1), torch.device("cuda"), cfg, logging.getLogger("test"), flip_test=False)
    assert set(metrics) == {"AP", "AP50", "AP75", "loss"}
