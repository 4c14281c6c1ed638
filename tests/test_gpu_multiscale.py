"""Multi-scale flip test on the device: pk_multiscale_merge against its numpy restatement (tests/multiscale_np.py) at the sizes where the
kernel's pixel loop and the inside rule change behaviour, the geometry on an affine ramp, the S = 1 identity with pk_flip_merge, and the
layers above it -- PoseEstimator.inference_multiscale through a padded twin (hrnet_w18, heatmap head) and the fusion head, and
DeviceBatcher(test_scales=)."""
import functools

import numpy as np
import pytest
import torch

import multiscale_np as msnp
from recipe import synth_input, synth_state_dict
from multiscale_np import PARTNER, ramp_stack, tolerance

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(i, i + 1) for i in range(1, 17, 2)]

# (H, W), scales: 9 x 7 = 63 pixels, fewer than the 256 threads of a workgroup; 20 x 15 = 300: the strided loop wraps with a ragged tail;
# 8 x 8 with exact inverses, where u_s lands exactly on the border 0 of the scale-0.5 pass (the inclusive border)
CASES = [((9, 7), (0.8, 1.0, 1.25)), ((20, 15), (0.75, 1.0, 1.25)), ((8, 8), (0.5, 1.0, 2.0))]


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached inputs are read-only


def C(t):
    return t.detach().float().cpu().numpy()


def _partner(K=3):
    return torch.tensor(PARTNER if K == 3 else _partner_of(PAIRS, K), dtype=torch.int32, device=DEV)


def _partner_of(pairs, K):
    p = list(range(K))
    for a, b in pairs:
        p[a], p[b] = b, a
    return p


@functools.lru_cache(maxsize=None)
def _random_stack(hw, S, F, B=2, K=3):
    a = np.random.default_rng(100 * S + F).standard_normal((S * F * B, K, *hw)).astype(np.float32)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("hw,scales", CASES + [(hw, (1.0,)) for hw, _ in CASES])
def test_kernel_equals_the_restatement(hw, scales, flip):
    from infantposeestimation_gaussianbias_amd import hipops
    msnp.assert_borders_are_decided_alike(hw, scales)
    S, F, B = len(scales), 2 if flip else 1, 2
    stack = _random_stack(hw, S, F)
    want = msnp.merge(stack, scales, B, PARTNER, flip)
    got = C(hipops.multiscale_merge(G(stack), scales, B, _partner() if flip else None, flip))
    err, tol = float(np.abs(got.astype(np.float64) - want).max()), tolerance(stack, S, F)
    print(f"{hw} scales {scales} F={F}: max |kernel - restatement| {err:.3e}, tolerance {tol:.3e}, bit-equal share {float((got == want).mean()):.4f}")
    assert got.shape == (B, 3, *hw) and err <= tol
    if S == 3:          # the passes really differ in what they see: some pixels have every pass, some have fewer
        seen = sum(np.outer((msnp.sample_coords(hw[0], i) >= 0) & (msnp.sample_coords(hw[0], i) <= hw[0] - 1),
                            (msnp.sample_coords(hw[1], i) >= 0) & (msnp.sample_coords(hw[1], i) <= hw[1] - 1)).astype(int) for i in msnp.inv_scales(scales))
        assert seen.max() == 3 and seen.min() < 3


def test_inclusive_border_on_the_device():
    """8 x 8, scales (0.5, 1.0, 2.0), constant maps 4 / 1 / 2: base pixels 2..5 see all three passes (u = 2 exactly on border 0 of the
    scale-0.5 pass), the rest only two -- exact values, so an exclusive border or a diluting divisor shows as a wrong constant."""
    from infantposeestimation_gaussianbias_amd import hipops
    stack = np.zeros((3, 1, 8, 8), np.float32)
    stack[0], stack[1], stack[2] = 4.0, 1.0, 2.0
    got = C(hipops.multiscale_merge(G(stack), (0.5, 1.0, 2.0), 1))[0, 0]
    seen = np.array([2 <= u <= 5 for u in range(8)])
    want = np.where(seen[:, None] & seen[None, :], np.float32(7.0) / np.float32(3.0), np.float32(1.5)).astype(np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("flip", [False, True])
def test_ramp_comes_back_on_the_device(flip):
    from infantposeestimation_gaussianbias_amd import hipops
    scales, B = (0.75, 1.0, 1.25), 2
    stack, want = ramp_stack(scales, B, 3, 20, 15, flip)
    got = C(hipops.multiscale_merge(G(stack), scales, B, _partner() if flip else None, flip))
    err, tol = float(np.abs(got.astype(np.float64) - want).max()), tolerance(stack, 3, 2 if flip else 1)
    print(f"ramp 20 x 15 flip {flip}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("hw", [(9, 7), (20, 15), (64, 48)])
def test_single_scale_flip_is_flip_merge_bitwise(hw):
    from infantposeestimation_gaussianbias_amd import hipops
    stack = G(_random_stack(hw, 1, 2))
    got = hipops.multiscale_merge(stack, (1.0,), 2, _partner(), True)
    want = hipops.flip_merge(stack[:2], stack[2:], _partner())
    assert torch.equal(got, want)
    assert torch.equal(hipops.multiscale_merge(stack, (1.0,), 4), stack)          # F = 1: the map itself


# ------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def _model(name):
    import json
    import os
    from conftest import GOLDEN
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        keys = json.load(f)
    bb, head, spec, salt = {"hrnet_w18": ("hrnet_w18", "heatmap", "hrnet_w18_heatmap", 41),
                            "hrformer_small": ("hrformer_small", "fusion", "hrformer_small_fusion", 40)}[name]
    m = PoseEstimator(bb, 17, False, head, True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(keys[spec], salt).items()}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", ["hrnet_w18", "hrformer_small"])
@pytest.mark.parametrize("flip", [False, True])
def test_one_scale_is_the_plain_inference_bitwise(name, flip):
    m = _model(name)
    x = G(synth_input("ms_one", (2, 3, 128, 96)))
    pairs = PAIRS if flip else None
    kp, sc = m.inference_multiscale([x], [1.0], flip, pairs)
    kp0, sc0 = m.inference(x, flip, pairs)
    assert kp.shape == (2, 17, 2) and torch.equal(kp, kp0) and torch.equal(sc, sc0)


@pytest.mark.parametrize("name", ["hrnet_w18", "hrformer_small"])
def test_three_scales_are_one_forward_in_pass_order_merged_and_decoded(name):
    """Three DIFFERENT random inputs per scale, the base crop last in the list: a wrong pass order, a wrong mirrored half or offsets taken
    from another pass than the un-flipped scale-1.0 one give other numbers.  Then the merged maps against the restatement of the merge."""
    from infantposeestimation_gaussianbias_amd import hipops
    m, scales, B = _model(name), (0.8, 1.25, 1.0), 2
    xs = [G(synth_input(f"ms_{i}", (B, 3, 128, 96))) for i in range(3)]
    kp, sc = m.inference_multiscale(xs, scales, True, PAIRS)
    kp5, sc5 = m.inference_multiscale(torch.stack(xs), scales, True, PAIRS)
    assert torch.equal(kp, kp5) and torch.equal(sc, sc5)                        # (S,B,3,H,W) and the list are the same call
    with torch.no_grad():
        out = m(torch.cat([t for x in xs for t in (x, torch.flip(x, dims=[-1]))], 0))
    hms = out["heatmaps"].float()
    H, W = hms.shape[2:]
    assert hms.shape[0] == 3 * 2 * B and (H, W) == (32, 24)
    msnp.assert_borders_are_decided_alike((H, W), scales)
    partner = torch.tensor(_partner_of(PAIRS, 17), dtype=torch.int32, device=DEV)
    hm = hipops.multiscale_merge(hms, scales, B, partner, True)
    decode = (lambda maps: m.head.decode({**{k: (v[4 * B:5 * B] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 6 * B else v)
                                             for k, v in out.items()}, "heatmaps": maps})) if name == "hrformer_small" else m.decode_heatmaps
    kp_w, sc_w = decode(hm)
    assert torch.equal(kp, kp_w) and torch.equal(sc, sc_w)
    # not the plain inference of the base crop, nor the merge with the base taken from another pass
    kp_b, sc_b = m.inference(xs[2], True, PAIRS)
    assert not torch.equal(sc, sc_b)
    ref = msnp.merge(C(hms), scales, B, _partner_of(PAIRS, 17), True)
    tol = tolerance(C(hms), 3, 2)
    err = float(np.abs(C(hm).astype(np.float64) - ref).max())
    kp_r, sc_r = decode(G(ref))
    dkp, dsc = float((kp - kp_r).abs().max()), float((sc - sc_r).abs().max())
    print(f"{name}: merged maps max |kernel - restatement| {err:.3e} (tolerance {tol:.3e}); through the decode: scores {dsc:.3e}, keypoints {dkp:.3e} px")
    assert err <= tol
    # scores are the maps' maxima (1-Lipschitz in the map): the same tolerance.  Keypoints: to first order the decode moves by at most
    # W * delta px for a map change delta (soft-argmax), or not at all (argmax away from ties); 1e-3 px is far above W * tol and far below
    # the jump of a changed argmax or rounding cell, which is what this line is there to catch
    assert dsc <= tol and dkp <= 1e-3


def test_training_mode_raises():
    m = _model("hrnet_w18")
    x = G(synth_input("ms_one", (2, 3, 128, 96)))
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.inference_multiscale([x], [1.0], False)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="1.0"):
        m.inference_multiscale([x, x], [0.8, 1.2], False)
    with pytest.raises(ValueError, match="S = 3"):
        m.inference_multiscale([x, x], [0.8, 1.0, 1.2], False)


# ------------------------------------------------------------------------------------------------ loader
def test_device_batcher_yields_the_crops_of_every_scale():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    from infantposeestimation_gaussianbias_amd.datasets.coco_dataset import DeviceBatcher
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (48, 64), (12, 16)
    rng, tf, recs = np.random.default_rng(21), T.get_val_transforms(cfg.data.input_size), []
    for i in range(3):
        H, W = int(rng.integers(60, 120)), int(rng.integers(50, 100))
        x1, y1, x2, y2 = W * 0.2, H * 0.15, W * 0.8, H * 0.9
        recs.append(tf({"center": np.array([(x1 + x2) / 2, (y1 + y2) / 2], np.float32), "scale": np.array([x2 - x1, y2 - y1], np.float32) * 1.25,
                        "keypoints": np.stack([rng.uniform(x1, x2, 17), rng.uniform(y1, y2, 17)], 1).astype(np.float32),
                        "keypoints_visible": np.ones(17, np.float32), "img": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "img_width": W,
                        "flip_pairs": PAIRS, "flip": False, "image_id": i, "ann_id": i, "bbox": np.array([x1, y1, x2, y2], np.float32),
                        "area": float((x2 - x1) * (y2 - y1))}))
    scales = (0.8, 1.2, 1.0)
    plain = next(iter(DeviceBatcher([recs], cfg, prefetch=False)))
    assert "img_scales" not in plain
    crop = T.DeviceCropper(cfg.data.input_size, DEV)
    for prefetch in (False, True):
        b = next(iter(DeviceBatcher([recs], cfg, prefetch=prefetch, test_scales=scales)))
        torch.cuda.synchronize()
        assert b["img_scales"].shape == (3, 3, 3, 64, 48)
        for i, s in enumerate(scales):
            mats = [T.multiscale_matrices(r["center"], r["scale"], scales, cfg.data.input_size)[i] for r in recs]
            want32, want16 = crop([r["img"] for r in recs], mats)
            assert torch.equal(b["img_scales"][i], want32), s
            if s == 1.0:
                assert torch.equal(b["img"], want32) and torch.equal(b["img_nhwc8"], want16)
        assert torch.equal(b["img"], plain["img"]) and torch.equal(b["target"], plain["target"])
        assert not torch.equal(b["img_scales"][0], b["img_scales"][2])
    with pytest.raises(ValueError):
        DeviceBatcher([recs], cfg, test_scales=(0.8, 1.2))


def test_validate_refuses_a_loader_without_the_scaled_crops():
    """validate(scales=) predicts from batch["img_scales"]; the synthetic loader has none, and there is no single-scale fallback."""
    import logging

    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import SyntheticLoader
    cfg = get_config("hrnet_w18")
    cfg.train.batch_size = 2
    with pytest.raises(RuntimeError, match="img_scales"):
        V.validate(_model("hrnet_w18"), SyntheticLoader(cfg, n_batches=1), torch.device(DEV), cfg, logging.getLogger("test"), flip_test=False,
                   scales=(0.8, 1.0, 1.2))


# ------------------------------------------------------------------------------------------------ inference.py
def test_pose_inference_crops_every_scale_once_and_maps_back_with_the_base_crop():
    import inference
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets.transforms import DeviceCropper, multiscale_matrices
    from infantposeestimation_gaussianbias_amd.utils.postprocess import heatmap_to_image_coords
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    pose = inference.PoseInference.__new__(inference.PoseInference)          # __init__ without the checkpoint handling, at a small input
    pose.device, pose.flip_test, pose.cfg, pose.model = torch.device(DEV), True, cfg, _model("hrformer_small")
    pose.input_size, pose.flip_pairs = cfg.data.input_size, cfg.data.flip_pairs
    pose._crop = DeviceCropper(pose.input_size, pose.device, nchw=True, nhwc8=False)
    img = np.random.default_rng(68).integers(0, 256, (96, 128, 3)).astype(np.uint8)
    boxes = [np.array([10.0, 8.0, 50.0, 60.0]), np.array([70.0, 30.0, 115.0, 90.0])]
    single = pose.predict_persons(img, boxes)
    pose.scales = (1.0,)
    one = pose.predict_persons(img, boxes)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(one, single))
    pose.scales = scales = (0.8, 1.0, 1.25)
    got, hm, centers, box_scales = pose.predict_persons(img, boxes, return_heatmaps=True)
    batch = pose.predict_batch([img, img], boxes)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, batch))
    cs = [pose._center_scale(img, b) for b in boxes]
    xs = [pose._crop([img], [multiscale_matrices(c, s, scales, pose.input_size)[i] for c, s in cs], None, bgr=True, image_index=[0, 0])[0]
          for i in range(3)]
    kp, sc = pose.model.inference_multiscale(xs, scales, True, pose.flip_pairs)
    c, s = (torch.from_numpy(np.stack([v[j] for v in cs]).astype(np.float32)).to(DEV) for j in (0, 1))
    want = heatmap_to_image_coords(kp, c, s, cfg.data.input_size, cfg.data.heatmap_size).cpu().numpy()
    assert all(np.array_equal(got[p][0], want[p]) and np.array_equal(got[p][1], sc[p].cpu().numpy()) for p in range(2))
    assert not np.array_equal(got[0][1], single[0][1])
    with torch.no_grad():
        base_hm = pose.model(xs[1])["heatmaps"].float()
    assert torch.equal(hm, base_hm) and np.array_equal(box_scales, np.stack([v[1] for v in cs]))


# ------------------------------------------------------------------------------------------------ validate.py over the COCO loader
def test_validate_predicts_from_the_scaled_crops_and_keeps_the_loss_on_the_base_crop(tmp_path):
    """Three small images with two persons each behind the COCO loader: with cfg.test_scales the loader yields img_scales and validate's
    predictions are those of inference_multiscale over them; the loss is still computed on `img`, the scale-1.0 crop, so it is the
    single-scale run's loss to the bit.  The training loader ignores the scales."""
    import json
    import logging
    import os

    from PIL import Image

    import coco_cases as cc
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import build_dataloader
    from infantposeestimation_gaussianbias_amd.utils.postprocess import heatmap_to_image_coords
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "val")
    images, anns = [], []
    for i in range(3):
        H, W = 160 + 20 * i, 140 + 10 * i
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / "val" / f"{i}.png")
        images.append({"id": 100 + i, "file_name": f"{i}.png", "width": W, "height": H})
        for j in range(2):
            anns.append(cc.gt_ann(1 + 2 * i + j, 100 + i, cc.pose(17, 20 + 50 * j, 30, 60, rng), 60 * 60 * 0.8 + 3000 * j, bbox=[15 + 50 * j, 25, 70, 70]))
    (tmp_path / "ann.json").write_text(json.dumps({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}))
    cfg = get_config("hrnet_w18")
    cfg.data.data_root, cfg.data.val_ann, cfg.data.val_img_prefix = str(tmp_path), "ann.json", "val/"
    cfg.data.train_ann, cfg.data.train_img_prefix = "ann.json", "val/"
    cfg.train.batch_size, cfg.train.num_workers = 2, 0
    model, log, dev = _model("hrnet_w18"), logging.getLogger("test"), torch.device(DEV)
    single, preds1 = V.validate(model, build_dataloader(cfg, is_train=False), dev, cfg, log, flip_test=True)
    cfg.test_scales = scales = (0.8, 1.0, 1.2)
    loader = build_dataloader(cfg, is_train=False)
    assert loader.test_scales == scales and build_dataloader(cfg, is_train=True).test_scales is None
    multi, preds = V.validate(model, loader, dev, cfg, log, flip_test=True, scales=scales)
    assert set(multi) == set(single) and multi["loss"] == single["loss"] and len(preds) == len(preds1) == 6
    assert [p["ann_id"] for p in preds] == [p["ann_id"] for p in preds1] and any(p["keypoints"] != q["keypoints"] for p, q in zip(preds, preds1))
    want = []
    for batch in loader:
        assert batch["img_scales"].shape == (3, batch["img"].shape[0], 3, 128, 96) and torch.equal(batch["img_scales"][1], batch["img"])
        kp, sc = model.inference_multiscale(batch["img_scales"], scales, True, cfg.data.flip_pairs)
        xy = heatmap_to_image_coords(kp, batch["meta"]["center"].to(dev), batch["meta"]["scale"].to(dev), cfg.data.input_size, cfg.data.heatmap_size)
        want += [np.concatenate([xy[b].cpu().numpy(), sc[b].cpu().numpy()[:, None]], 1).reshape(-1).tolist() for b in range(kp.shape[0])]
    assert [p["keypoints"] for p in preds] == want
