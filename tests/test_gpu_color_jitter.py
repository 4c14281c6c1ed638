"""Colour jitter on the device (pk_affine_crop_jitter_normalize through DeviceCropper / DeviceBatcher) against the numpy model of its
arithmetic (tests/jitter_np.py, bit for bit) and against the reference's CustomColorJitter outputs (tests/golden/color_jitter.npz,
within the cap the model itself is held to)."""
import functools

import numpy as np
import pytest
import torch

import jitter_np

pytestmark = pytest.mark.gpu

PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
IDENTITY = np.array([[1., 0, 0], [0, 1., 0]])
CAP_SHARE, CAP_DIFF = 1e-3, 1       # vs the reference: at most 1 apart on at most 0.1 % of the bytes (a condition, not a measurement)


def _record(rng, H, W, K=17):
    x1, y1 = rng.uniform(0, W * 0.4), rng.uniform(0, H * 0.4)
    x2, y2 = x1 + rng.uniform(W * 0.3, W * 0.55), y1 + rng.uniform(H * 0.3, H * 0.55)
    kp = np.stack([rng.uniform(x1, x2, K), rng.uniform(y1, y2, K)], 1).astype(np.float32)
    vis = rng.choice([0.0, 1.0, 2.0], K, p=[0.2, 0.3, 0.5]).astype(np.float32)
    return {"center": np.array([(x1 + x2) / 2, (y1 + y2) / 2], np.float32), "scale": np.array([x2 - x1, y2 - y1], np.float32) * 1.25,
            "keypoints": kp, "keypoints_visible": vis}


JITTER = [(1.21, 0.78, 1.15), None, (0.74, 1.27, 0.83), None, (1.05, 1.3, 1.2)]       # two of five disabled


@functools.lru_cache(maxsize=None)
def _ragged(w, h):
    """The ragged batch of test_device_cropper_bit_exact_vs_oracle (different source sizes, flips, rotations, a crop that is mostly border)
    with B = 5, and the model's output for it; computed once per crop size and never modified."""
    from oracle import warp as ow
    rng = np.random.default_rng(3)
    imgs, mats, flips, want = [], [], [], []
    for i in range(5):
        H, W = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rec = _record(rng, H, W)
        if i == 0:
            rec["center"], rec["scale"] = np.array([2., 3.], np.float32), np.array([W * 1.5, H * 1.5], np.float32)      # mostly border
        info = ow.train_sample(img, rec, (w, h), np.random.RandomState(i), flip_pairs=PAIRS)[3]
        imgs.append(img)
        mats.append(info["matrix"])
        flips.append(bool(info["flip"]))
        want.append(jitter_np.crop_jitter_normalize(img, info["matrix"], (w, h), flip=info["flip"], jitter=JITTER[i]))
    assert any(flips) and not all(flips)
    want = np.stack(want)
    want.setflags(write=False)
    return imgs, mats, flips, want


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("w,h", [(48, 64), (20, 13)])
def test_ragged_batch_is_bit_equal_to_the_model(w, h):
    """(48, 64): 12 workgroups per sample, so the walk over the partial sums has more than one term.  (20, 13): 260 pixels, i.e. a second
    workgroup with 4 live threads -- its 252 idle threads must add nothing to S.  Both outputs; disabled samples equal the plain call."""
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    imgs, mats, flips, want = _ragged(w, h)
    crop = T.DeviceCropper((w, h), "cuda")
    out32, out16 = crop(imgs, mats, flips, jitter=JITTER)
    plain32, plain16 = crop(imgs, mats, flips)
    torch.cuda.synchronize()
    got = _bits(out32)
    for i in range(len(imgs)):
        assert np.array_equal(got[i], want[i].view(np.uint32)), f"sample {i} (jitter {JITTER[i]}) differs from the model"
    ref16 = torch.from_numpy(want.copy()).permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(out16[..., :3].cpu(), ref16) and float(out16[..., 3:].abs().max()) == 0.0
    for i, j in enumerate(JITTER):
        same32, same16 = torch.equal(out32[i], plain32[i]), torch.equal(out16[i], plain16[i])
        assert (same32 and same16) if j is None else (not same32 and not same16), f"sample {i}: bypass / jitter mixed up"
    # BGR source: the same crops of the channel-swapped images
    o_bgr, none16 = T.DeviceCropper((w, h), "cuda", nhwc8=False)([im[:, :, ::-1].copy() for im in imgs], mats, flips, bgr=True, jitter=JITTER)
    assert none16 is None and torch.equal(o_bgr, out32)
    only16 = T.DeviceCropper((w, h), "cuda", nchw=False)(imgs, mats, flips, jitter=JITTER)
    assert only16[0] is None and torch.equal(only16[1], out16)
    # all-None takes the existing call
    calls = []
    orig = T.call
    try:
        T.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        off32, _ = crop(imgs, mats, flips, jitter=[None] * len(imgs))
    finally:
        T.call = orig
    assert calls == ["pk_affine_crop_normalize"] and torch.equal(off32, plain32)


def test_corner_factors_are_bit_equal_to_the_model():
    """One 16 x 12 crop: c = 0 (every value is m), s = 0 (gray), b = 1.6 / c = 2 / s = 2 (both clamps), identity factors (not the identity),
    and a constant image."""
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    from oracle import warp as ow
    img = np.random.default_rng(8).integers(0, 256, (16, 12, 3), dtype=np.uint8)
    const = np.full((16, 12, 3), 137, np.uint8)
    imgs = [img, img, img, img, const]
    factors = [(1.1, 0.0, 1.3), (0.9, 1.2, 0.0), (1.6, 2.0, 2.0), (1.0, 1.0, 1.0), (0.8, 1.3, 0.7)]
    out32, out16 = T.DeviceCropper((12, 16), "cuda")(imgs, [IDENTITY] * 5, jitter=factors)
    torch.cuda.synchronize()
    got = out32.cpu().numpy()
    for i, (im, f) in enumerate(zip(imgs, factors)):
        u8 = jitter_np.jitter_u8(im, *f)
        assert np.array_equal(got[i].view(np.uint32), ow.normalize_chw(u8).view(np.uint32)), f"factors {f}"
        back = jitter_np.denormalize_to_u8(got[i])
        if i in (0, 4):
            assert len(np.unique(back)) == 1
        if i == 1:
            assert np.array_equal(back[..., 0], back[..., 1]) and np.array_equal(back[..., 1], back[..., 2])
        if i == 2:
            assert (back == 0).any() and (back == 255).any()
        if i == 3:
            assert (back != im).any()
    assert torch.equal(out16[..., :3].cpu(), torch.from_numpy(got).permute(0, 2, 3, 1).to(torch.bfloat16))


def test_fixture_crops_match_the_reference_class_within_the_cap(golden):
    """The reference's CustomColorJitter outputs: fixture crops through the device path with an identity matrix at the crop's own size,
    de-normalised back to bytes through the model's table."""
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    g = golden("color_jitter.npz")
    by_size = {}
    for n in g["names"]:
        by_size.setdefault(g[f"{n}.img"].shape, []).append(str(n))
    assert len(by_size) >= 2
    for (h, w, _), names in by_size.items():
        out32, _ = T.DeviceCropper((w, h), "cuda", nhwc8=False)([g[f"{n}.img"] for n in names], [IDENTITY] * len(names),
                                                                jitter=[tuple(g[f"{n}.factors"]) for n in names])
        got = out32.cpu().numpy()
        for i, n in enumerate(names):
            diff = np.abs(jitter_np.denormalize_to_u8(got[i]).astype(np.int32) - g[f"{n}.out"].astype(np.int32))
            print(f"{n}: {float((diff > 0).mean()):.2e} of the bytes differ from the reference, max {int(diff.max())}")
            assert diff.max() <= CAP_DIFF and (diff > 0).mean() <= CAP_SHARE, n


def _record_loader(n_batches, B, cfg, seed=11):
    """Record lists as the COCO DataLoader hands them to DeviceBatcher, with jitter decisions drawn by the transform."""
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    rng = np.random.default_rng(seed)
    tf = T.Compose([T.TopdownAffine(cfg.data.input_size), T.ColorJitter(0.3, 0.3, 0.2, prob=0.6, rng=np.random.RandomState(seed))])
    batches = []
    for _ in range(n_batches):
        recs = []
        for i in range(B):
            H, W = int(rng.integers(120, 220)), int(rng.integers(100, 180))
            r = _record(rng, H, W)
            r.update(img=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), img_width=W, flip_pairs=PAIRS, flip=False, image_id=i, ann_id=i,
                     bbox=np.array([0, 0, W, H], np.float32), area=float(H * W))
            recs.append(tf(r))
        batches.append(recs)
    return batches


def test_jitter_is_deterministic_and_prefetch_equals_the_synchronous_path():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    from infantposeestimation_gaussianbias_amd.datasets.coco_dataset import DeviceBatcher
    imgs, mats, flips, _ = _ragged(48, 64)
    crop = T.DeviceCropper((48, 64), "cuda")
    a32, a16 = crop(imgs, mats, flips, jitter=JITTER)
    b32, b16 = crop(imgs, mats, flips, jitter=JITTER)
    assert torch.equal(a32, b32) and torch.equal(a16, b16)
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    loader = _record_loader(4, 6, cfg)
    flags = [s["jitter"] is not None for b in loader for s in b]
    assert any(flags) and not all(flags)
    keep = lambda b: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    want = [keep(b) for b in DeviceBatcher(loader, cfg, prefetch=False)]
    got = []
    for i, b in enumerate(DeviceBatcher(loader, cfg, prefetch=True)):
        if i % 2:
            torch.cuda.synchronize()
        got.append(keep(b))
    plain = [keep(b) for b in DeviceBatcher([[dict(s, jitter=None) for s in b] for b in loader], cfg, prefetch=False)]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for a, b, p, recs in zip(got, want, plain, loader):
        for k in ("img", "img_nhwc8", "target", "target_weight", "keypoints", "keypoints_visible"):
            assert torch.equal(a[k], b[k]), k
        for i, s in enumerate(recs):                      # the batcher passed the records' decisions on
            assert torch.equal(b["img"][i], p["img"][i]) == (s["jitter"] is None)


def test_argument_errors_raise_before_any_launch():
    from infantposeestimation_gaussianbias_amd import _lib
    from infantposeestimation_gaussianbias_amd._lib import call, stream_ptr
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    imgs, mats, flips, _ = _ragged(48, 64)
    with pytest.raises(_lib.PoseKernelError):
        T.DeviceCropper((48, 64), "cuda")(imgs, mats, flips, jitter=JITTER[:4])
    with pytest.raises(_lib.PoseKernelError, match="2\\^32"):
        T.DeviceCropper((4096, 2048), "cuda")(imgs[:1], mats[:1], jitter=[(1.0, 1.0, 1.0)])
    # the C entry refuses the same shape, and a workspace that is too small, by itself
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.PoseKernelError, match="2\\^32"):
        call("pk_affine_crop_jitter_normalize", buf, buf, buf, 1, 4096, 2048, out, None, T.MEAN.ctypes.data, T.STD.ctypes.data, buf, 4096, stream_ptr())
    with pytest.raises(_lib.PoseKernelError, match="workspace"):
        call("pk_affine_crop_jitter_normalize", buf, buf, buf, 1, 48, 64, out, None, T.MEAN.ctypes.data, T.STD.ctypes.data, buf, 4096, stream_ptr())
    torch.cuda.synchronize()
