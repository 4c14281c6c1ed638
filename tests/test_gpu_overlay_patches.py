"""Per-person heatmap overlay on the device (pk_heatmap_overlay_patches through hipops / utils/visualization.py / inference.py) against
the float64 restatement of tests/overlay_patches_np.py; the shared upload of DeviceCropper(image_index=) and PoseInference.predict_persons
against the calls that send the image once per person."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_patches_np as opn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _V():
    from infantposeestimation_gaussianbias_amd.utils import visualization
    return visualization


def _lut():
    return torch.from_numpy(_V().heatmap_lut()).to(DEV)


def _overlay(images, hm, idx, mats, alpha=0.5):
    """-> (blended batch, index, cover) as numpy."""
    from infantposeestimation_gaussianbias_amd import hipops
    batch = torch.from_numpy(images).to(DEV)
    index, cover = hipops.heatmap_overlay_patches(batch, torch.from_numpy(np.asarray(hm, np.float32)).to(DEV), idx, mats, alpha, _lut(),
                                                  want_index=True, want_cover=True)
    return batch.cpu().numpy(), index.cpu().numpy(), cover.cpu().numpy()


def test_index_and_cover_planes_against_float64():
    """idx = floor(255 v) with v from max over K, the bilinear sample at the float64-mapped position and the patch's own normalisation.
    As in test_heatmap_index_plane_against_float64 the float32 chain is about ten roundings of 2^-24 relative on a value <= 255 (~1.5e-4
    absolute): wherever the float64 value 255 v is farther than 1e-3 from an integer the indices must be equal, elsewhere they may differ
    by one; the share of covered pixels in that band is printed and must stay below 2 % (the restatement alone on these inputs: 0.2 %,
    test_overlay_patches_host.py).  Covered / uncovered is decided in float64 on both sides and must agree everywhere; the blend is
    integer and must equal draw_np.overlay_blend of the device's own index plane."""
    N, H, W = opn.FRAMES
    images = np.random.default_rng(61).integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    for case in opn.comparison_cases():
        mats = opn.case_matrices(case)
        got, index, cover = _overlay(images, case["heatmaps"], case["image_index"], mats)
        assert index.shape == cover.shape == (N, H, W) and index.dtype == cover.dtype == np.uint8
        banded = covered = 0
        for n in range(N):
            v, want_cover, _ = opn.overlay_patches_f64(H, W, case["heatmaps"], case["image_index"], mats, n)
            assert np.array_equal(cover[n], want_cover), f"frame {n}: {(cover[n] != want_cover).sum()} cover counts differ"
            on = want_cover > 0
            want = opn.index_of(v, want_cover)
            band = on & (np.abs(v - np.rint(v)) <= 1e-3)
            banded, covered = banded + int(band.sum()), covered + int(on.sum())
            g = index[n].astype(np.int64)
            assert np.array_equal(g[~band], want[~band]), f"frame {n}: {(g[~band] != want[~band]).sum()} indices differ outside the rounding band"
            assert np.abs(g - want).max() <= 1
            blend = opn.overlay_blend(images[n], index[n], opn.jet_lut(), 0.5)
            assert np.array_equal(got[n][on], blend[on]) and np.array_equal(got[n][~on], images[n][~on])
        assert index.max() > 128, "the case draws next to nothing"
        share = banded / covered
        print(f"P = {len(mats)}: share of covered pixels within 1e-3 of an integer index boundary: {share:.5f}")
        assert share < 0.02


def test_identity_matrix_gives_the_float32_index_exactly():
    """h x w equal to the frame and the identity matrix: every pixel samples one tap with fraction 0, so the index is the float32
    expression itself -- no band."""
    H, W, K = 37, 53, 5
    hm = opn.blobs(62, 1, K, H, W)
    images = np.random.default_rng(63).integers(0, 256, (1, H, W, 3)).astype(np.uint8)
    _, index, cover = _overlay(images, hm, [0], np.array([[1.0, 0, 0, 0, 1.0, 0]]))
    m = hm[0].max(axis=0)
    lo, hi = m.min(), m.max()
    v = (m - lo) / ((hi - lo) + np.float32(1e-8))
    assert v.dtype == np.float32
    want = np.clip(np.floor(np.float32(255.0) * v), 0, 255).astype(np.uint8)
    assert np.array_equal(index[0], want) and (cover == 1).all() and want.max() >= 254 and want.min() == 0


def test_peak_lands_where_the_decode_puts_it():
    """A patch whose only non-zero value is 1.0 at an integer heat pixel: the frame pixel nearest to heatmap_to_image_coords of that heat
    pixel carries the frame's maximum index (scale aspect = input aspect, where the decode's per-axis scale and the crop matrix agree)."""
    from infantposeestimation_gaussianbias_amd.utils.postprocess import heatmap_to_image_coords
    V = _V()
    H, W, (w, h), input_size = 150, 203, (48, 64), (192, 256)
    center, scale, (hx, hy) = np.array([101.3, 71.8]), np.array([90.0, 120.0]), (29, 17)
    hm = np.zeros((1, 17, h, w), np.float32)
    hm[0, 3, hy, hx] = 1.0
    xy = heatmap_to_image_coords(torch.tensor([[[hx, hy]]], dtype=torch.float32, device=DEV), torch.from_numpy(center[None]),
                                 torch.from_numpy(scale[None]), input_size, (w, h)).cpu().numpy()[0, 0]
    nx, ny = int(np.rint(xy[0])), int(np.rint(xy[1]))
    assert abs(xy[0] - nx) < 0.45 and abs(xy[1] - ny) < 0.45 and 0 <= nx < W and 0 <= ny < H, "the case has a tie between two pixels"
    images = np.zeros((1, H, W, 3), np.uint8)
    _, index, _ = _overlay(images, hm, [0], V.crop_heatmap_matrices([center], [scale], (w, h)))
    assert index.max() > 128 and index[0, ny, nx] == index.max()
    assert (index[0] == index.max()).sum() == 1


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_alpha_endpoints(alpha):
    N, H, W = opn.FRAMES
    case = opn.comparison_cases()[0]
    images = np.random.default_rng(64).integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    got, index, cover = _overlay(images, case["heatmaps"], case["image_index"], opn.case_matrices(case), alpha)
    if alpha == 0.0:
        assert np.array_equal(got, images)
    else:
        on = cover > 0
        assert np.array_equal(got[on], opn.jet_lut()[index[on]]) and np.array_equal(got[~on], images[~on]) and on.any()


def test_draw_poses_lays_person_heatmaps_underneath_and_is_reproducible():
    V = _V()
    N, H, W = opn.FRAMES
    case = opn.comparison_cases()[0]
    rng = np.random.default_rng(65)
    images = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    kp = np.stack([rng.uniform(20, 180, (5, 17)), rng.uniform(20, 130, (5, 17))], -1).astype(np.float32)
    sc = rng.uniform(0.31, 1.0, (5, 17)).astype(np.float32)
    boxes, bidx = np.array([[20.5, 15.25, 130.0, 100.0], [40, 30, 190, 140]], np.float32), [0, 2]
    batch = torch.from_numpy(images).to(DEV)
    hm = torch.from_numpy(case["heatmaps"]).to(DEV)
    pat = dict(heatmap_centers=case["centers"], heatmap_scales=case["scales"], heatmap_rotations=case["rotations"])
    run = lambda: V.draw_poses(batch, kp, sc, case["image_index"], boxes=boxes, box_image_index=bidx, heatmaps=hm, alpha=0.3, **pat)   # noqa: E731
    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)
    second = run()
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(batch.cpu(), torch.from_numpy(images))
    under = V.draw_person_heatmaps(batch, hm, centers=case["centers"], scales=case["scales"], rotations=case["rotations"],
                                   image_index=case["image_index"], alpha=0.3)
    assert not torch.equal(under, batch) and torch.equal(under[1], batch[1])
    assert torch.equal(first, V.draw_poses(under, kp, sc, case["image_index"], boxes=boxes, box_image_index=bidx))
    # the matrices themselves are accepted in place of centers / scales, and one person on one numpy image needs no index
    assert torch.equal(under, V.draw_person_heatmaps(batch, hm, matrices=opn.case_matrices(case), image_index=case["image_index"], alpha=0.3))
    one = V.draw_person_heatmaps(images[0], case["heatmaps"][0], centers=case["centers"][0], scales=case["scales"][0], alpha=0.3)
    want = V.draw_person_heatmaps(batch[:1], hm[:1], centers=case["centers"][:1], scales=case["scales"][:1], image_index=[0], alpha=0.3)
    assert isinstance(one, np.ndarray) and np.array_equal(one, want[0].cpu().numpy())


def test_wrapper_refuses_a_bad_index_or_matrix_and_draws_nothing_for_no_patches():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    images = np.random.default_rng(66).integers(0, 256, (2, 20, 40, 3)).astype(np.uint8)
    batch = torch.from_numpy(images).to(DEV)
    hm = torch.rand(2, 3, 8, 6, device=DEV)
    mats = np.tile(np.array([[0.2, 0, 0, 0, 0.2, 0]]), (2, 1))
    for idx in ([1, 0], [0, 2], [-1, 0]):
        with pytest.raises(PoseKernelError, match="image_index"):
            hipops.heatmap_overlay_patches(batch, hm, idx, mats, 0.5, _lut())
    bad = mats.copy()
    bad[1, 2] = np.nan
    with pytest.raises(PoseKernelError, match="finite"):
        hipops.heatmap_overlay_patches(batch, hm, [0, 1], bad, 0.5, _lut())
    with pytest.raises(PoseKernelError):
        hipops.heatmap_overlay_patches(batch, hm, [0], mats, 0.5, _lut())
    assert torch.equal(batch.cpu(), torch.from_numpy(images)), "a refused call drew something"
    index, cover = hipops.heatmap_overlay_patches(batch, hm[:0], [], np.zeros((0, 6)), 0.5, _lut(), want_index=True, want_cover=True)
    assert torch.equal(batch.cpu(), torch.from_numpy(images)) and int(index.max()) == 0 and int(cover.max()) == 0
    assert hipops.heatmap_overlay_patches(batch, hm, [0, 1], mats, 0.5, _lut()) == (None, None)
    assert not torch.equal(batch.cpu(), torch.from_numpy(images))


@pytest.mark.parametrize("augment", [False, True])
def test_device_cropper_shares_one_upload_between_crops(augment):
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    from infantposeestimation_gaussianbias_amd.datasets.transforms import DeviceCropper, get_affine_matrix
    rng = np.random.default_rng(67)
    a, b = (rng.integers(0, 256, (60, 80, 3)).astype(np.uint8) for _ in range(2))
    mats = [get_affine_matrix(np.array(c), np.array(s), (24, 32), r) for c, s, r in
            (((30.5, 28.0), (45.0, 60.0), 0.0), ((52.2, 33.1), (30.0, 40.0), 20.0), ((40.0, 30.0), (60.0, 80.0), -10.0))]
    flips = [False, True, True] if augment else None
    jitter = [(1.1, 0.9, 1.2), None, (0.8, 1.15, 0.9)] if augment else None
    crop = DeviceCropper((24, 32), DEV)
    want32, want16 = crop([a, a, b], mats, flips, jitter=jitter)
    got32, got16 = crop([a, b], mats, flips, jitter=jitter, image_index=[0, 0, 1])
    assert got32.shape == (3, 3, 32, 24) and got16.shape == (3, 32, 24, 8)
    assert torch.equal(got32, want32) and torch.equal(got16.view(torch.int16), want16.view(torch.int16))
    for bad in ([0, 2, 1], [0, -1, 1], [0, 1]):
        with pytest.raises(PoseKernelError):
            crop([a, b], mats, flips, jitter=jitter, image_index=bad)


def test_predict_persons_equals_predict_batch_and_its_heatmaps_stay_inside_the_crops():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import inference
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets.transforms import DeviceCropper
    from infantposeestimation_gaussianbias_amd.models import build_model
    V = _V()
    torch.manual_seed(0)
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    pose = inference.PoseInference.__new__(inference.PoseInference)          # __init__ without the checkpoint handling, at a small input
    pose.device, pose.flip_test, pose.cfg = torch.device(DEV), True, cfg
    pose.model = build_model(cfg).to(DEV).eval()
    pose.input_size, pose.flip_pairs = cfg.data.input_size, cfg.data.flip_pairs
    pose._crop = DeviceCropper(pose.input_size, pose.device, nchw=True, nhwc8=False)
    H, W = 96, 128
    img = np.random.default_rng(68).integers(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = [np.array([10.0, 8.0, 50.0, 60.0]), np.array([70.0, 30.0, 115.0, 90.0])]
    want = pose.predict_batch([img, img], boxes)
    got, hm, centers, scales = pose.predict_persons(img, boxes, return_heatmaps=True)
    assert len(got) == 2 and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, want))
    plain = pose.predict_persons(img, boxes)
    assert all(np.array_equal(g[0], p[0]) and np.array_equal(g[1], p[1]) for g, p in zip(got, plain))
    assert tuple(hm.shape) == (2, cfg.model.num_keypoints, 32, 24) and centers.shape == scales.shape == (2, 2)
    vis = pose.visualize_batch(img[None], [[]], heatmaps=hm, heatmap_centers=centers, heatmap_scales=scales)[0]
    inside = np.zeros((H, W), bool)
    mats = V.crop_heatmap_matrices(centers, scales, (24, 32))
    for p in range(2):
        inside |= opn.overlay_patches_f64(H, W, hm[p:p + 1].cpu().numpy(), [0], mats[p:p + 1], 0)[1] > 0
    changed = (vis != img).any(-1)
    assert changed.any() and not (changed & ~inside).any() and inside.sum() < 0.8 * H * W
    # with the poses on top it is the same picture as drawing them over that overlay
    full = pose.visualize_batch(img[None], [got], heatmaps=hm, heatmap_centers=centers, heatmap_scales=scales)[0]
    assert np.array_equal(full, pose.visualize_batch(vis[None], [got])[0])
