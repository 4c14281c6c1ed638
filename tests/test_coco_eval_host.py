"""COCO keypoint AP / AR, host side (no GPU): the numpy restatement against hand-derived results, the host preparation of COCOKeypointEval
(ignore flags, detection areas, id and sigma checks) and the argument checks of the new C-ABI entries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import coco_cases as cc  # noqa: E402
import cocoeval_np  # noqa: E402


def _close(got, want, tol=1e-12):
    assert set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_restatement_reproduces_the_hand_derived_cases(case):
    ann, recs, want = getattr(cc, f"case_{case}")()
    stats, prec, rec, ious, _ = cocoeval_np.cocoeval(ann, recs, cc.COCO_SIGMAS)
    _close(stats, want)
    if case == "a":
        oks = ious[1][0, 0]
        assert 0.70 < oks < 0.75
        assert np.all(rec[:5, 0] == 1) and np.all(rec[5:, 0] == 0)
    if case == "b":
        assert np.allclose(prec[:, :51, 0], 1, atol=1e-12) and np.allclose(prec[:, 51:, 0], 2 / 3, atol=1e-12)


def test_restatement_takes_the_later_of_two_equal_ground_truths():
    ann, recs = cc.case_d()
    _, _, _, ious, evalImgs = cocoeval_np.cocoeval(ann, recs, cc.COCO_SIGMAS)
    assert ious[5][0, 0] == ious[5][0, 1] == 1.0
    assert np.all(evalImgs[0][0]['dtGt'] == 1)


def test_restatement_box_distance_oks_without_visible_joints():
    ann, recs, want = cc.case_e()
    _, _, _, ious, _ = cocoeval_np.cocoeval(ann, recs, cc.COCO_SIGMAS)
    assert ious[9][:, 0].tolist() == want


def test_np_sum_order_is_numpys():
    """The pairwise order pk_eval.hip follows for the OKS sum (< 8 terms left to right; 8 strided partial sums, combined pairwise, then the
    tail) is what np.sum does for every length the kernel meets (K <= 64)."""
    rng = np.random.default_rng(0)
    for n in range(1, 65):
        for _ in range(20):
            v = np.exp(-rng.uniform(0, 30, n)) * rng.uniform(0.5, 2, n)
            assert cocoeval_np.np_sum_order(v) == np.sum(v), n


def test_host_preparation_ignore_flags_and_areas():
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import COCOKeypointEval
    kp = cc.pose(17, 10, 20, 100)
    anns = [cc.gt_ann(1, 2, kp, 5000), cc.gt_ann(2, 2, kp, 5000, iscrowd=1), cc.gt_ann(3, 1, kp, 5000, num_keypoints=0),
            cc.gt_ann(4, 2, kp, 5000, ignore=1), cc.gt_ann(5, 1, kp, 5000)]
    del anns[4]['num_keypoints'], anns[4]['iscrowd']          # missing: counted from v > 0 / 0
    ev = COCOKeypointEval(cc.dataset([2, 1], anns), cc.COCO_SIGMAS)
    assert ev.img_ids.tolist() == [1, 2]
    assert ev.gt_ids.tolist() == [3, 5, 1, 2, 4]               # grouped by sorted image id, file order inside an image
    assert (ev.gt_flags & 1).tolist() == [1, 0, 0, 1, 0]       # num_keypoints 0 / crowd ignored; the file's 'ignore' key has no effect
    assert (ev.gt_flags >> 1).tolist() == [0, 0, 0, 1, 0]
    assert ev.gt_off.tolist() == [0, 2, 5]
    det = kp.copy()
    det[:, 0] = np.linspace(3, 13, 17)
    det[:, 1] = np.linspace(-1, 6, 17)
    recs = [cc.rec(2, det, 0.5), cc.rec(1, kp, 0.7), cc.rec(2, kp, 0.1)]
    idx, dkp, score, area, dt_off = ev.prepare_detections(recs)
    assert idx.tolist() == [1, 0, 2] and dt_off.tolist() == [0, 1, 3]
    assert area[1] == (13 - 3) * (6 - -1)                      # keypoint extent, the record's own area is not used
    assert score.tolist() == [0.7, 0.5, 0.1]


def test_host_preparation_rejects_bad_input():
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import COCOKeypointEval
    kp = cc.pose(17, 10, 20, 100)
    ev = COCOKeypointEval(cc.dataset([1], [cc.gt_ann(1, 1, kp, 5000)]), cc.COCO_SIGMAS)
    with pytest.raises(ValueError, match="image_id 7"):
        ev.prepare_detections([cc.rec(1, kp, 0.5), cc.rec(7, kp, 0.5)])
    with pytest.raises(ValueError, match="sigma"):
        COCOKeypointEval(cc.dataset([1], [cc.gt_ann(1, 1, kp[:13], 5000)], K=13), cc.COCO_SIGMAS)
    COCOKeypointEval(cc.dataset([1], [cc.gt_ann(1, 1, kp[:13], 5000)], K=13), np.full(13, 0.05))      # K = 13 with its own sigmas
    two = cc.dataset([1], [cc.gt_ann(1, 1, kp, 5000)])
    two['categories'].append({'id': 2, 'name': 'other'})
    with pytest.raises(ValueError, match="category"):
        COCOKeypointEval(two, cc.COCO_SIGMAS)
    with pytest.raises(ValueError, match="id 0"):
        COCOKeypointEval(cc.dataset([1], [cc.gt_ann(0, 1, kp, 5000)]), cc.COCO_SIGMAS)


def test_empty_inputs_give_cocoeval_results_without_a_launch():
    """No records: areas holding non-ignored ground truth get precision / recall 0, the others -1; no ground truth at all: -1 everywhere.
    Neither case reaches the device, so this runs without one."""
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import COCOKeypointEval
    kp = cc.pose(17, 10, 20, 100)
    ev = COCOKeypointEval(cc.dataset([1], [cc.gt_ann(1, 1, kp, 5000)]), cc.COCO_SIGMAS)
    stats = ev.evaluate([])
    assert stats == {'AP': 0.0, 'AP50': 0.0, 'AP75': 0.0, 'AP_M': 0.0, 'AP_L': -1.0, 'AR': 0.0, 'AR50': 0.0, 'AR75': 0.0, 'AR_M': 0.0,
                     'AR_L': -1.0}
    ev = COCOKeypointEval(cc.dataset([1, 2], []), cc.COCO_SIGMAS)
    assert set(ev.evaluate([cc.rec(2, kp, 0.3)]).values()) == {-1.0}


def test_coco_entry_points_reject_null_and_zero_arguments():
    from infantposeestimation_gaussianbias_amd import _lib
    L = _lib.lib
    rc = L.pk_coco_kpt_oks(*([None] * 12), 1, 17, 20, None)
    assert rc == -1 and b"null pointer" in L.pk_last_error_string()
    p = 16                                                      # any non-NULL value: the size checks run before anything is read
    rc = L.pk_coco_kpt_oks(*([p] * 12), 0, 17, 20, None)
    assert rc == -1 and b"bad size" in L.pk_last_error_string()
    rc = L.pk_coco_kpt_oks(*([p] * 12), 1, 65, 20, None)
    assert rc == -2 and b"built for" in L.pk_last_error_string()
    rc = L.pk_coco_kpt_eval(*([None] * 19), 1, 1, 1, 3, 10, 101, None)
    assert rc == -1 and b"null pointer" in L.pk_last_error_string()
    rc = L.pk_coco_kpt_eval(*([p] * 19), 1, 1, 0, 3, 10, 101, None)
    assert rc == -1 and b"bad size" in L.pk_last_error_string()
    rc = L.pk_coco_kpt_eval(*([p] * 19), 1, 1, 1, 7, 10, 101, None)
    assert rc == -2 and b"built for" in L.pk_last_error_string()
    assert L.pk_coco_kpt_eval_ws_floats(0, 0, 0, 0) == 0
    assert L.pk_coco_kpt_eval_ws_floats(10, 100, 3, 10) * 4 >= 30 * 10 + 30 * 100 * 12
