"""Detector-box validation without a GPU: the numpy restatement of rescoring / OKS-NMS (tests/oks_nms_np.py) on hand cases with known
answers, the two new entries of the header (argument counts, statuses and messages of their argument checks: nothing is launched), the op
layer's checks, the dataset built from a detection file, the legacy-yaml mapping of the TEST block and validate.py's flags."""
import ctypes
import dataclasses
import json
import logging
import math

import numpy as np
import pytest
import torch

import oks_nms_np as onp

VARS17 = (2.0 * onp.COCO_SIGMAS) ** 2


def _pose(x0, y0, scores=0.9, K=17):
    kp = np.zeros((K, 3))
    kp[:, 0], kp[:, 1], kp[:, 2] = x0 + 7.0 * np.arange(K), y0 + 3.0 * np.arange(K), scores
    return kp


def _one_image(poses, scores, areas=None):
    kpt = np.stack(poses)
    n = len(poses)
    return kpt, np.full(n, 5000.0) if areas is None else np.asarray(areas, float), np.asarray(scores, float), np.array([0, n], np.int32)


# ------------------------------------------------------------------------------------------------ the restatement on hand cases
def test_of_two_identical_poses_the_lower_scored_one_goes():
    kpt, area, score, off = _one_image([_pose(10, 20), _pose(10, 20), _pose(400, 300)], [0.6, 0.8, 0.7])
    keep, n_keep, order, out, margin = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.9, 0.2)
    assert keep.tolist() == [0, 1, 1] and n_keep.tolist() == [2]
    assert order.tolist() == [1, 2, -1]                     # selection order: by descending score
    assert out.tolist() == [0.0, 0.8, 0.7]
    # compared: 1-2 (far: oks ~ 0), 1-0 (identical: oks 1), 2-0 is not (0 is gone) -> the nearest to 0.9 is the 1.0
    assert abs(margin - 0.1) <= 1e-12


def test_equal_scores_the_lower_index_survives():
    kpt, area, score, off = _one_image([_pose(10, 20), _pose(10, 20)], [0.5, 0.5])
    keep, n_keep, order, _, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.9, 0.2)
    assert keep.tolist() == [1, 0] and order.tolist() == [0, -1] and n_keep.tolist() == [1]


def test_without_a_common_confident_joint_oks_is_zero_and_both_stay():
    a, b = _pose(10, 20), _pose(10, 20)
    a[:, 2] = np.where(np.arange(17) % 2 == 0, 0.9, 0.1)    # confident on the even joints
    b[:, 2] = np.where(np.arange(17) % 2 == 1, 0.9, 0.1)    # ... and on the odd ones: same place, nothing in common
    kpt, area, score, off = _one_image([a, b], [0.9, 0.8])
    assert onp.oks_to(a, 5000.0, b[None], np.array([5000.0]), VARS17, 0.2).tolist() == [0.0]
    keep, _, order, _, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.5, 0.2)
    assert keep.tolist() == [1, 1] and order.tolist() == [0, 1]
    # with the threshold at -inf every joint counts and the two are the same pose
    keep, _, _, _, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.5, -math.inf)
    assert keep.tolist() == [1, 0]


def test_strict_comparison_and_nan_scores_last():
    kpt, area, score, off = _one_image([_pose(10, 20), _pose(10, 20), _pose(10, 20)], [math.nan, 0.3, 0.2])
    keep, _, order, out, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 1.0, 0.2)       # oks == 1 is not > 1: nothing goes
    assert keep.tolist() == [1, 1, 1] and order.tolist() == [1, 2, 0] and math.isnan(out[0])
    keep, _, order, _, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.9, 0.2)
    assert keep.tolist() == [0, 1, 0] and order.tolist() == [1, -1, -1]


def test_soft_mode_with_oks_zero_leaves_scores_untouched_and_ties_resolve_by_index():
    a, b, c = _pose(10, 20), _pose(10, 20), _pose(10, 20)
    a[:, 2] = np.where(np.arange(17) < 6, 0.9, 0.1)         # three disjoint sets of confident joints: every OKS is exactly 0
    b[:, 2] = np.where((np.arange(17) >= 6) & (np.arange(17) < 12), 0.9, 0.1)
    c[:, 2] = np.where(np.arange(17) >= 12, 0.9, 0.1)
    kpt, area, score, off = _one_image([a, b, c], [0.4, 0.7, 0.7])
    keep, n_keep, order, out, margin = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.5, 0.2, soft=True, max_dets=20)
    assert keep.tolist() == [1, 1, 1] and n_keep.tolist() == [3]
    assert order.tolist() == [1, 2, 0]                      # the tie 0.7 / 0.7 goes to the lower index
    assert out.tolist() == [0.4, 0.7, 0.7]                  # exp(-0 / thr) == 1 exactly
    assert abs(margin - (0.7 - 0.4) / 0.7) <= 1e-15         # the tie itself is excluded from the margin
    keep, n_keep, order, out, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.5, 0.2, soft=True, max_dets=2)
    assert keep.tolist() == [0, 1, 1] and order.tolist() == [1, 2, -1] and out.tolist() == [0.0, 0.7, 0.7]


def test_soft_mode_decays_a_duplicate_by_exp_minus_one_over_thr():
    kpt, area, score, off = _one_image([_pose(10, 20), _pose(10, 20), _pose(400, 300)], [0.9, 0.8, 0.5])
    keep, _, order, out, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.5, 0.2, soft=True, max_dets=20)
    # 0 is selected; its duplicate 1 decays to 0.8 exp(-1 / 0.5) = 0.108 and falls behind 2 (far away: untouched to 1e-300)
    assert order.tolist() == [0, 2, 1]
    assert abs(out[1] - 0.8 * math.exp(-2.0)) <= 1e-15 and abs(out[2] - 0.5) <= 1e-15
    with pytest.raises(ValueError):
        onp.oks_nms_np(kpt, area, score, off, VARS17, 0.0, 0.2, soft=True)


def test_images_are_independent_and_empty_ones_keep_nothing():
    p = [_pose(10, 20), _pose(10, 20)]
    kpt, area, score = np.stack(p + p), np.full(4, 5000.0), np.array([0.9, 0.8, 0.3, 0.4])
    off = np.array([0, 0, 2, 2, 4, 4], np.int32)
    keep, n_keep, order, _, _ = onp.oks_nms_np(kpt, area, score, off, VARS17, 0.9, 0.2)
    assert n_keep.tolist() == [0, 1, 0, 1, 0] and keep.tolist() == [1, 0, 0, 1] and order.tolist() == [0, -1, 1, -1]


def test_rescore_is_box_score_times_the_mean_confident_keypoint_score():
    kpt = np.zeros((3, 4, 3))
    kpt[0, :, 2] = [0.5, 0.1, 0.9, 0.2]        # 0.2 is not > 0.2
    kpt[1, :, 2] = [0.1, 0.0, 0.2, 0.05]       # nothing qualifies
    kpt[2, :, 2] = [0.25, 0.75, 0.5, 1.0]
    got = onp.rescore_np(kpt, np.array([0.5, 0.9, 2.0]), 0.2)
    assert got.tolist() == [0.5 * ((0.5 + 0.9) / 2), 0.0, 2.0 * ((((0.25 + 0.75) + 0.5) + 1.0) / 4)]
    assert onp.rescore_np(kpt, None, 0.2).tolist() == [(0.5 + 0.9) / 2, 0.0, 0.625]
    assert onp.rescore_np(kpt, None, -math.inf)[1] == ((0.1 + 0.0) + 0.2 + 0.05) / 4


def test_generator_meets_its_conditions_on_a_small_batch():
    """The conditions the GPU test asserts for every seeded case, on one of them (they are properties of the data, so they hold or fail
    here exactly as there): margin, at least 10 % removed and at least 50 % kept in the images of 20 and more poses."""
    kpt, area, score, off, vars_ = onp.make_batch((0, 3, 20, 65), 17, 0, tie=True)
    keep, n_keep, _, _, margin = onp.oks_nms_np(kpt, area, score, off, vars_, 0.9, 0.2)
    assert margin >= 1e-9
    for n, k in zip(np.diff(off), n_keep):
        if n >= 20:
            assert n - k >= 0.1 * n and k >= 0.5 * n
    assert len(set(score[off[2]:off[3]].tolist())) == 19          # exactly one tied pair


# ------------------------------------------------------------------------------------------------ the C-ABI's argument checks
def _lib():
    from infantposeestimation_gaussianbias_amd import _lib as L
    return L


def test_header_declares_both_entries_with_their_arguments():
    sym = _lib().declared_symbols()
    ret, args = sym["pk_pose_rescore"]
    assert ret == "int" and len(args) == 7
    assert args == [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    ret, args = sym["pk_oks_nms"]
    assert ret == "int" and len(args) == 16
    assert args == [ctypes.c_void_p] * 9 + [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p]
    assert hasattr(_lib().lib, "pk_pose_rescore") and hasattr(_lib().lib, "pk_oks_nms")


def test_argument_checks_return_statuses_with_messages():
    """Every refusal happens before anything touches the device: fake non-NULL pointers are never dereferenced."""
    L = _lib().lib
    err = lambda: L.pk_last_error_string().decode()
    P = 4096                                                   # any non-NULL value
    assert L.pk_pose_rescore(None, None, None, 0, 0, 0.2, None) == -1 and "null pointer" in err()
    assert L.pk_pose_rescore(P, None, None, 4, 17, 0.2, None) == -1 and "null pointer" in err()
    assert L.pk_pose_rescore(P, None, P, 0, 17, 0.2, None) == -1 and "bad size" in err()
    assert L.pk_pose_rescore(P, None, P, 4, 0, 0.2, None) == -1 and "bad size" in err()
    assert L.pk_pose_rescore(P, None, P, 4, 65, 0.2, None) == -1 and "K 65" in err()
    assert L.pk_pose_rescore(P, None, P, 4, 17, math.nan, None) == -1 and "NaN" in err()
    nine = [P] * 9
    assert L.pk_oks_nms(*[None] * 9, 0, 0, 0.0, 0.0, 0, 0, None) == -1 and "null pointer" in err()
    for i in range(9):                                         # each pointer on its own
        ptrs = list(nine)
        ptrs[i] = None
        assert L.pk_oks_nms(*ptrs, 2, 17, 0.9, 0.2, 0, 20, None) == -1 and "null pointer" in err(), i
    assert L.pk_oks_nms(*nine, 0, 17, 0.9, 0.2, 0, 20, None) == -1 and "n_img 0" in err()
    assert L.pk_oks_nms(*nine, -3, 17, 0.9, 0.2, 0, 20, None) == -1 and "n_img -3" in err()
    assert L.pk_oks_nms(*nine, 2, 0, 0.9, 0.2, 0, 20, None) == -1 and "K 0" in err()
    assert L.pk_oks_nms(*nine, 2, 65, 0.9, 0.2, 0, 20, None) == -1 and "K 65" in err()
    for bad in (math.nan, math.inf, -math.inf):
        assert L.pk_oks_nms(*nine, 2, 17, bad, 0.2, 0, 20, None) == -1 and "finite" in err(), bad
    assert L.pk_oks_nms(*nine, 2, 17, 0.9, math.nan, 0, 20, None) == -1 and "in_vis_thr" in err()
    assert L.pk_oks_nms(*nine, 2, 17, 0.0, 0.2, 1, 20, None) == -1 and "soft mode" in err()
    assert L.pk_oks_nms(*nine, 2, 17, -0.5, 0.2, 1, 20, None) == -1 and "soft mode" in err()
    assert L.pk_oks_nms(*nine, 2, 17, 0.9, 0.2, 1, 0, None) == -1 and "max_dets" in err()


def test_op_layer_checks_shapes_and_refuses_cpu_tensors():
    from infantposeestimation_gaussianbias_amd import _lib as L, hipops
    kp, ar, sc, va = torch.zeros(4, 17, 3, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), \
        torch.ones(17, dtype=torch.float64)
    off = np.array([0, 4], np.int32)
    with pytest.raises(ValueError, match="kpt"):
        hipops.oks_nms(kp[:, :, :2], ar, sc, off, va, 0.9)
    with pytest.raises(ValueError, match="area"):
        hipops.oks_nms(kp, ar[:3], sc, off, va, 0.9)
    with pytest.raises(ValueError, match="vars"):
        hipops.oks_nms(kp, ar, sc, off, va[:5], 0.9)
    with pytest.raises(ValueError, match="off"):
        hipops.oks_nms(kp, ar, sc, np.array([0, 3], np.int32), va, 0.9)
    with pytest.raises(ValueError, match="off"):
        hipops.oks_nms(kp, ar, sc, np.array([0, 4], np.int64), va, 0.9)
    with pytest.raises(ValueError, match="soft"):
        hipops.oks_nms(kp, ar, sc, off, va, 0.0, soft=True)
    with pytest.raises(ValueError, match="keypoints"):
        hipops.oks_nms(torch.zeros(4, 65, 3, dtype=torch.float64), ar, sc, off, torch.ones(65, dtype=torch.float64), 0.9)
    with pytest.raises(L.PoseKernelError, match="CUDA"):                    # shapes are fine: the device / dtype check is what refuses
        hipops.oks_nms(kp, ar, sc, off, va, 0.9)
    with pytest.raises(ValueError, match="box_score"):
        hipops.pose_rescore(kp, torch.ones(3, dtype=torch.float64))
    with pytest.raises(L.PoseKernelError, match="CUDA"):
        hipops.pose_rescore(kp, None)
    # the per-image limit is checked on the host, before any device work: the message names the image and its count
    n = hipops.OKS_NMS_MAX_POSES + 1
    with pytest.raises(L.PoseKernelError, match=r"PK_ERR_UNSUPPORTED.*image 1 holds 1025 poses"):
        hipops.oks_nms(torch.zeros(n + 2, 17, 3, dtype=torch.float64), torch.ones(n + 2, dtype=torch.float64),
                       torch.ones(n + 2, dtype=torch.float64), np.array([0, 2, n + 2], np.int32), va, 0.9)


def test_public_functions_are_exported():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd.utils import postprocess
    assert utils.oks_nms is postprocess.oks_nms and utils.soft_oks_nms is postprocess.soft_oks_nms
    assert "oks_nms" in utils.__all__ and "soft_oks_nms" in utils.__all__
    with pytest.raises(ValueError, match="sigma"):
        postprocess._oks_nms(torch.zeros(2, 13, 3), torch.ones(2), torch.ones(2), 0.9, None, 0.2, None, False, 0)


def test_evaluator_keeps_box_scores_and_its_old_behaviour():
    from infantposeestimation_gaussianbias_amd.utils import COCOEvaluator
    ev = COCOEvaluator(num_keypoints=17)
    assert ev.oks_nms_thr is None and ev.in_vis_thr == 0.2 and ev.soft_nms is False and ev.nms_max_dets == 20 and ev.kept == []
    kp, sc = np.zeros((2, 17, 2)), np.full((2, 17), 0.5)
    ev.update(kp, sc, [1, 1], [-1, -1], areas=[10.0, 20.0], bboxes=np.zeros((2, 4)), box_scores=[0.9, 0.25])
    assert [r["box_score"] for r in ev.predictions] == [0.9, 0.25]
    ev.update(kp, sc, [1, 1], [5, 6], areas=[10.0, 20.0], bboxes=np.zeros((2, 4)))
    assert "box_score" not in ev.predictions[2]
    ev.reset()
    assert ev.predictions == [] and ev.kept == []


# ------------------------------------------------------------------------------------------------ dataset from a detection file
def _files(root):
    images = [{"id": 7, "file_name": "a.png", "width": 200, "height": 100}, {"id": 9, "file_name": "b.png", "width": 120, "height": 160}]
    ann = {"images": images, "annotations": [], "categories": [{"id": 1, "name": "person"}]}
    (root / "ann.json").write_text(json.dumps(ann))
    dets = [
        {"image_id": 7, "category_id": 1, "bbox": [10, 20, 50, 60], "score": 0.9},         # 0: kept as it is
        {"image_id": 7, "category_id": 1, "bbox": [10, 20, 50, 60], "score": 0.2},         # below the score threshold
        {"image_id": 7, "category_id": 3, "bbox": [10, 20, 50, 60], "score": 0.95},        # not a person
        {"image_id": 8, "category_id": 1, "bbox": [10, 20, 50, 60], "score": 0.95},        # image not in the annotation file
        {"image_id": 9, "category_id": 1, "bbox": [-10, 130, 60, 50], "score": 0.3},       # 1: clipped to [0, 130, 50, 160]; score == threshold
        {"image_id": 9, "category_id": 1, "bbox": [130, 10, 20, 20], "score": 0.8},        # outside the image after clipping
        {"image_id": 9, "category_id": 1, "bbox": [10, 10, 0, 20], "score": 0.8},          # zero width
        {"image_id": 9, "category_id": 1, "bbox": [100, 100, 40, 40], "score": 0.7},       # 2: clipped to [100, 100, 120, 140]
    ]
    (root / "dets.json").write_text(json.dumps(dets))


def test_dataset_reads_detector_boxes(tmp_path):
    from infantposeestimation_gaussianbias_amd.datasets.coco_dataset import COCOPoseDataset
    _files(tmp_path)
    ds = COCOPoseDataset(str(tmp_path), "ann.json", "val/", is_train=False, bbox_file="dets.json", det_score_thr=0.3)
    assert len(ds) == 3
    assert [r["image_id"] for r in ds.db] == [7, 9, 9] and all(r["ann_id"] == -1 for r in ds.db)
    assert [r["box_score"] for r in ds.db] == [0.9, 0.3, 0.7]
    assert [r["bbox"].tolist() for r in ds.db] == [[10, 20, 60, 80], [0, 130, 50, 160], [100, 100, 120, 140]]
    assert [r["area"] for r in ds.db] == [50.0 * 60.0, 50.0 * 30.0, 20.0 * 40.0]
    assert ds.db[1]["center"].tolist() == [25.0, 145.0] and ds.db[1]["scale"].tolist() == [62.5, 37.5]
    for r in ds.db:
        assert r["keypoints"].shape == (17, 2) and not r["keypoints"].any() and r["keypoints_visible"].shape == (17,) \
            and not r["keypoints_visible"].any()
        assert r["image_file"].endswith(("a.png", "b.png"))
    # no threshold: the low-scored box is back; the ground-truth path is unchanged (no annotations: no records, no box_score)
    assert len(COCOPoseDataset(str(tmp_path), "ann.json", "val/", is_train=False, bbox_file="dets.json")) == 4
    assert len(COCOPoseDataset(str(tmp_path), "ann.json", "val/", is_train=False)) == 0
    # an absolute path is taken as it is
    assert len(COCOPoseDataset(str(tmp_path / "elsewhere"), str(tmp_path / "ann.json"), "val/", is_train=False,
                               bbox_file=str(tmp_path / "dets.json"))) == 4


def test_dataset_refuses_a_missing_or_malformed_detection_file(tmp_path):
    from infantposeestimation_gaussianbias_amd.datasets.coco_dataset import COCOPoseDataset
    _files(tmp_path)
    mk = lambda name: COCOPoseDataset(str(tmp_path), "ann.json", "val/", is_train=False, bbox_file=name)
    with pytest.raises(ValueError, match="nothere.json"):
        mk("nothere.json")
    (tmp_path / "broken.json").write_text("[{")
    with pytest.raises(ValueError, match="broken.json"):
        mk("broken.json")
    (tmp_path / "dict.json").write_text(json.dumps({"detections": []}))
    with pytest.raises(ValueError, match="dict.json"):
        mk("dict.json")
    (tmp_path / "nobox.json").write_text(json.dumps([{"image_id": 7, "category_id": 1, "score": 0.9}]))
    with pytest.raises(ValueError, match="nobox.json.*detection 0"):
        mk("nobox.json")
    (tmp_path / "short.json").write_text(json.dumps([{"image_id": 7, "category_id": 1, "score": 0.9, "bbox": [1, 2, 3]}]))
    with pytest.raises(ValueError, match="short.json"):
        mk("short.json")
    with pytest.raises(ValueError, match="validation"):
        COCOPoseDataset(str(tmp_path), "ann.json", "val/", is_train=True, bbox_file="dets.json")


# ------------------------------------------------------------------------------------------------ config and command line
def test_config_attributes_are_not_dataclass_fields():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.configs.config import Config
    cfg = get_config()
    assert (cfg.bbox_file, cfg.det_score_thr, cfg.oks_nms_thr, cfg.in_vis_thr, cfg.soft_nms) == (None, 0.0, None, 0.2, False)
    names = {f.name for f in dataclasses.fields(Config)}
    assert names == {"data", "model", "train", "exp_name", "seed"}


def test_legacy_yaml_test_block(tmp_path, caplog):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    p = tmp_path / "det.yaml"
    p.write_text("TEST:\n  USE_GT_BBOX: false\n  COCO_BBOX_FILE: dets/person.json\n  IMAGE_THRE: 0.1\n  OKS_THRE: 0.9\n  IN_VIS_THRE: 0.25\n"
                 "  SOFT_NMS: true\nEVAL:\n  OKS_THRESHOLD: 0.5\n")
    with caplog.at_level(logging.INFO):
        cfg = get_config(str(p))
    assert (cfg.bbox_file, cfg.det_score_thr, cfg.oks_nms_thr, cfg.in_vis_thr, cfg.soft_nms) == ("dets/person.json", 0.1, 0.9, 0.25, True)
    assert not [r for r in caplog.records if "USE_GT_BBOX" in r.getMessage()]
    # EVAL.OKS_THRESHOLD is a match threshold, not an NMS threshold
    q = tmp_path / "gt.yaml"
    q.write_text("TEST:\n  USE_GT_BBOX: false\nEVAL:\n  OKS_THRESHOLD: 0.5\n")
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cfg = get_config(str(q))
    assert (cfg.bbox_file, cfg.det_score_thr, cfg.oks_nms_thr, cfg.in_vis_thr, cfg.soft_nms) == (None, 0.0, None, 0.2, False)
    said = [r.getMessage() for r in caplog.records if "USE_GT_BBOX" in r.getMessage()]
    assert len(said) == 1 and "ground-truth boxes" in said[0]
    # the class attributes of other configs are untouched by the one that set its own
    assert get_config().oks_nms_thr is None and get_config().bbox_file is None


def test_command_line_flags_parse_and_reach_the_config():
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    a = V.build_parser().parse_args(["--checkpoint", "c.pth"])
    assert (a.bbox_file, a.det_score_thr, a.oks_nms, a.soft_nms, a.in_vis_thr) == (None, None, None, False, None)
    cfg = V.apply_detector_box_args(get_config(), a)
    assert (cfg.bbox_file, cfg.det_score_thr, cfg.oks_nms_thr, cfg.in_vis_thr, cfg.soft_nms) == (None, 0.0, None, 0.2, False)
    a = V.build_parser().parse_args(["--checkpoint", "c.pth", "--bbox_file", "dets.json", "--det_score_thr", "0.05", "--oks_nms", "0.9",
                                     "--soft_nms", "--in_vis_thr", "0.3"])
    cfg = V.apply_detector_box_args(get_config(), a)
    assert (cfg.bbox_file, cfg.det_score_thr, cfg.oks_nms_thr, cfg.in_vis_thr, cfg.soft_nms) == ("dets.json", 0.05, 0.9, 0.3, True)
    with pytest.raises(ValueError, match="oks_nms"):
        V.apply_detector_box_args(get_config(), V.build_parser().parse_args(["--checkpoint", "c.pth", "--soft_nms"]))
    with pytest.raises(SystemExit):
        V.build_parser().parse_args(["--checkpoint", "c.pth", "--oks_nms"])
