"""Occlusion, blur and noise on the device (pk_affine_crop_augment_normalize through DeviceCropper / DeviceBatcher) against the numpy
restatement of its arithmetic (tests/augment_np.py, bit for bit: the stages are integer work, the jitter and the normalisation are
the contracts of tests/jitter_np.py and oracle/warp.py), and properties that need no restatement."""
import functools

import numpy as np
import pytest
import torch

import augment_np as anp
import jitter_np

pytestmark = pytest.mark.gpu

PAIRS = [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)]
IDENTITY = np.array([[1., 0, 0], [0, 1., 0]])


def _record(rng, H, W, K=17):
    x1, y1 = rng.uniform(0, W * 0.4), rng.uniform(0, H * 0.4)
    x2, y2 = x1 + rng.uniform(W * 0.3, W * 0.55), y1 + rng.uniform(H * 0.3, H * 0.55)
    kp = np.stack([rng.uniform(x1, x2, K), rng.uniform(y1, y2, K)], 1).astype(np.float32)
    vis = rng.choice([0.0, 1.0, 2.0], K, p=[0.2, 0.3, 0.5]).astype(np.float32)
    return {"center": np.array([(x1 + x2) / 2, (y1 + y2) / 2], np.float32), "scale": np.array([x2 - x1, y2 - y1], np.float32) * 1.25,
            "keypoints": kp, "keypoints_visible": vis}


def _everything(w, h):
    """Four rectangles: the first two overlap, the second reaches outside the crop, the third is empty after clipping, both modes occur;
    the fourth lies over the second (a later one overwrites an earlier one)."""
    return {"blur": 1.7, "noise": (8.0, 20240117),
            "occlusion": {"rects": [(1, 2, w // 2, h // 2), (w // 3, h // 4, w + 9, h - 3), (-8, -8, 0, 6), (w // 2 - 2, h // 2 - 2, w // 2 + 3, h // 2 + 4)],
                          "mode": [0, 1, 0, 0], "rgb": [(124, 116, 104), (0, 0, 0), (255, 0, 0), (3, 200, 77)], "seed": 77}}


JITTER = [None, (1.21, 0.78, 1.15), None, (0.74, 1.27, 0.83), None, (1.05, 1.3, 1.2)]


def _decisions(w, h):
    """all off; jitter only; blur sigma 0.3 (R = 1); blur sigma 2.5 (R = 7) + jitter; noise only; everything on."""
    return [None, None, {"blur": 0.3}, {"blur": 2.5}, {"noise": (6.0, 424242)}, _everything(w, h)]


@functools.lru_cache(maxsize=None)
def _ragged(w, h):
    """A ragged batch of six (different source sizes, flips, rotations, one crop that is mostly border) and the restatement's output for it;
    computed once per crop size and never modified."""
    from oracle import warp as ow
    rng = np.random.default_rng(3)
    imgs, mats, flips, want = [], [], [], []
    dec = _decisions(w, h)
    for i in range(6):
        H, W = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rec = _record(rng, H, W)
        if i == 0:
            rec["center"], rec["scale"] = np.array([2., 3.], np.float32), np.array([W * 1.5, H * 1.5], np.float32)      # mostly border
        info = ow.train_sample(img, rec, (w, h), np.random.RandomState(i), flip_pairs=PAIRS)[3]
        imgs.append(img)
        mats.append(info["matrix"])
        flips.append(bool(info["flip"]))
        want.append(anp.crop_augment_normalize(img, info["matrix"], (w, h), flip=info["flip"], jitter=JITTER[i], decision=dec[i]))
    want = np.stack(want)
    want.setflags(write=False)
    return imgs, mats, flips, want


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _T():
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    return T


@pytest.mark.parametrize("w,h", [(48, 64), (20, 13)])
def test_ragged_batch_is_bit_equal_to_the_restatement(w, h):
    """(48, 64): 2 x 2 tiles of 32 x 32, the second column half filled, so halos cross tile borders in both directions.  (20, 13): narrower
    and lower than a tile, a partly filled last tile row.  Both outputs; the all-off sample equals the plain call's bits, the jitter-only
    sample the jitter call's."""
    T = _T()
    imgs, mats, flips, want = _ragged(w, h)
    dec = _decisions(w, h)
    crop = T.DeviceCropper((w, h), "cuda")
    calls, orig = [], T.call
    try:
        T.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        out32, out16 = crop(imgs, mats, flips, jitter=JITTER, augment=dec)
        plain32, plain16 = crop(imgs, mats, flips)
        jit32, jit16 = crop(imgs, mats, flips, jitter=JITTER)
    finally:
        T.call = orig
    torch.cuda.synchronize()
    assert calls == ["pk_affine_crop_augment_normalize", "pk_affine_crop_normalize", "pk_affine_crop_jitter_normalize"]
    got = _bits(out32)
    for i in range(len(imgs)):
        assert np.array_equal(got[i], want[i].view(np.uint32)), f"sample {i} (jitter {JITTER[i]}, {dec[i]}) differs from the restatement"
    ref16 = torch.from_numpy(want.copy()).permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(out16[..., :3].cpu(), ref16) and float(out16[..., 3:].abs().max()) == 0.0
    assert torch.equal(out32[0], plain32[0]) and torch.equal(out16[0], plain16[0])                 # everything off
    assert torch.equal(out32[1], jit32[1]) and torch.equal(out16[1], jit16[1]) and not torch.equal(out32[1], plain32[1])      # jitter only
    for i in range(2, 6):
        assert not torch.equal(out32[i], jit32[i]) and not torch.equal(out16[i], jit16[i]), f"sample {i}: stages skipped"
    # one output at a time, and a BGR source
    only32 = T.DeviceCropper((w, h), "cuda", nhwc8=False)([im[:, :, ::-1].copy() for im in imgs], mats, flips, bgr=True, jitter=JITTER, augment=dec)
    assert only32[1] is None and torch.equal(only32[0], out32)
    only16 = T.DeviceCropper((w, h), "cuda", nchw=False)(imgs, mats, flips, jitter=JITTER, augment=dec)
    assert only16[0] is None and torch.equal(only16[1], out16)
    # without a jitter list the rows' jitter fields are off
    nj32, _ = crop(imgs, mats, flips, augment=dec)
    torch.cuda.synchronize()
    for i in (0, 2, 4):
        assert torch.equal(nj32[i], out32[i])
    assert np.array_equal(_bits(nj32[3]), anp.crop_augment_normalize(imgs[3], mats[3], (w, h), flip=flips[3], decision=dec[3]).view(np.uint32))


def test_every_clamp_at_once_on_a_crop_smaller_than_the_radius():
    """(7, 5) with R = 7: every tap row and column of every pixel runs into the clamp, on all four sides."""
    T = _T()
    rng = np.random.default_rng(12)
    imgs = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8) for _ in range(3)]
    dec = [{"blur": 2.5}, {"blur": 2.5, "noise": (10.0, 5)}, {"blur": [128, 64]}]
    jit = [None, (1.1, 0.9, 1.2), None]
    out32, out16 = T.DeviceCropper((7, 5), "cuda")(imgs, [IDENTITY] * 3, jitter=jit, augment=dec)
    torch.cuda.synchronize()
    for i in range(3):
        want = anp.crop_augment_normalize(imgs[i], IDENTITY, (7, 5), jitter=jit[i], decision=dec[i])
        assert np.array_equal(_bits(out32[i]), want.view(np.uint32)), i
    assert torch.equal(out16[..., :3].cpu(), out32.cpu().permute(0, 2, 3, 1).to(torch.bfloat16))


def test_impulse_constant_and_full_fill_properties():
    """No restatement: the impulse response at an interior pixel and at the corner, a constant image under blur, and one constant
    rectangle over the whole crop."""
    T = _T()
    from oracle import warp as ow
    w, h, sigma = 40, 37, 1.7                        # two tiles in both directions
    q = [int(v) for v in T.blur_weights(sigma)]
    R = len(q) - 1
    inner, corner = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    inner[30, 33] = 255                              # next to the tile border at 32: its response crosses it
    corner[0, 0] = 255
    const = np.full((h, w, 3), (17, 137, 255), np.uint8)
    noisy = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    fill = {"occlusion": {"rects": [(-5, -5, w + 5, h + 5)], "mode": 0, "rgb": (124, 116, 104), "seed": 0}, "blur": sigma, "noise": (9.0, 3)}
    out32, _ = T.DeviceCropper((w, h), "cuda", nhwc8=False)([inner, corner, const, noisy], [IDENTITY] * 4,
                                                           augment=[{"blur": sigma}, {"blur": sigma}, {"blur": sigma}, fill])
    got = [jitter_np.denormalize_to_u8(o) for o in out32.cpu().numpy()]
    one = lambda i, j: ((((255 * q[abs(i)] + 128) >> 8) * q[abs(j)] + 128) >> 8)
    for i in range(-R, R + 1):
        for j in range(-R, R + 1):
            assert np.all(got[0][30 + j, 33 + i] == one(i, j)), (i, j)
    assert got[0].astype(np.int64).sum() == 3 * sum(one(i, j) for i in range(-R, R + 1) for j in range(-R, R + 1))      # and nothing else
    # at the corner the clamp folds the taps that fall outside onto the edge: the weight of pixel 0 in pass output x is the sum of q[|k|]
    # over the taps k with clamp(x + k) = 0
    fold = [sum(q[abs(k)] for k in range(-R, R + 1) if max(x + k, 0) == 0) for x in range(R + 1)]
    for x in range(R + 1):
        for y in range(R + 1):
            assert np.all(got[1][y, x] == ((((255 * fold[x] + 128) >> 8) * fold[y] + 128) >> 8)), (x, y)
    assert np.array_equal(got[2], const)
    assert np.all(got[3] == (124, 116, 104))
    assert np.array_equal(out32[3].cpu().numpy().view(np.uint32), ow.normalize_chw(np.full((h, w, 3), (124, 116, 104), np.uint8)).view(np.uint32))


def test_no_decision_takes_the_calls_and_gives_the_bits_of_before():
    T = _T()
    imgs, mats, flips, _ = _ragged(48, 64)
    crop = T.DeviceCropper((48, 64), "cuda")
    plain32, plain16 = crop(imgs, mats, flips)
    jit32, jit16 = crop(imgs, mats, flips, jitter=JITTER)
    calls, orig = [], T.call
    try:
        T.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        a32, a16 = crop(imgs, mats, flips, augment=[None] * 6)
        b32, b16 = crop(imgs, mats, flips, jitter=JITTER, augment=[None, {}, {"blur": None}, None, {"noise": None, "occlusion": None}, None])
        c32, _ = crop(imgs, mats, flips, jitter=[None] * 6, augment=None)
    finally:
        T.call = orig
    torch.cuda.synchronize()
    assert calls == ["pk_affine_crop_normalize", "pk_affine_crop_jitter_normalize", "pk_affine_crop_normalize"]
    assert torch.equal(a32, plain32) and torch.equal(a16, plain16) and torch.equal(b32, jit32) and torch.equal(b16, jit16) and torch.equal(c32, plain32)


def _record_loader(n_batches, B, cfg, seed=11):
    """Record lists as the COCO DataLoader hands them to DeviceBatcher, with the decisions drawn by the transforms."""
    T = _T()
    rng, rs = np.random.default_rng(seed), np.random.RandomState(seed)
    tf = T.Compose([T.TopdownAffine(cfg.data.input_size), T.ColorJitter(0.3, 0.3, 0.2, prob=0.5, rng=rs), T.RandomBlur(0.5, (0.3, 2.0), rng=rs),
                    T.SensorNoise(0.5, (2.0, 10.0), rng=rs),
                    T.RandomOcclusion(0.5, 3, (0.02, 0.2), (0.3, 3.3), "random", rng=rs, input_size=cfg.data.input_size)])
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


def test_deterministic_prefetch_equals_synchronous_and_labels_do_not_change():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets.coco_dataset import DeviceBatcher
    T = _T()
    imgs, mats, flips, _ = _ragged(48, 64)
    dec = _decisions(48, 64)
    crop = T.DeviceCropper((48, 64), "cuda")
    a32, a16 = crop(imgs, mats, flips, jitter=JITTER, augment=dec)
    b32, b16 = crop(imgs, mats, flips, jitter=JITTER, augment=dec)
    assert torch.equal(a32, b32) and torch.equal(a16, b16)
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    loader = _record_loader(3, 6, cfg)
    decided = [any(s[k] is not None for k in ("blur", "noise", "occlusion")) for b in loader for s in b]
    assert any(decided) and not all(decided)
    keep = lambda b: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}
    want = [keep(b) for b in DeviceBatcher(loader, cfg, prefetch=False)]
    got = []
    for i, b in enumerate(DeviceBatcher(loader, cfg, prefetch=True)):
        if i % 2:
            torch.cuda.synchronize()
        got.append(keep(b))
    clean = [keep(b) for b in DeviceBatcher([[dict(s, blur=None, noise=None, occlusion=None) for s in b] for b in loader], cfg, prefetch=False)]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 3
    for a, b, c, recs in zip(got, want, clean, loader):
        for k in ("img", "img_nhwc8", "target", "target_weight", "keypoints", "keypoints_visible"):
            assert torch.equal(a[k], b[k]), k
        for k in ("target", "target_weight", "keypoints", "keypoints_visible"):      # the labels of the clean sample
            assert torch.equal(b[k], c[k]), k
        for i, s in enumerate(recs):                                                # the batcher passed the records' decisions on
            assert torch.equal(b["img"][i], c["img"][i]) == all(s[k] is None for k in ("blur", "noise", "occlusion")), i
    # a batch without any decision takes the jitter call, as before
    calls, orig = [], T.call
    try:
        T.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        next(iter(DeviceBatcher([[dict(s, blur=None, noise=None, occlusion=None, jitter=(1.1, 0.9, 1.0)) for s in loader[0]]], cfg, prefetch=False)))
    finally:
        T.call = orig
    assert [c for c in calls if c.startswith("pk_affine_crop")] == ["pk_affine_crop_jitter_normalize"]


def test_cropper_raises_before_staging():
    T = _T()
    from infantposeestimation_gaussianbias_amd import _lib
    imgs, mats, flips, _ = _ragged(48, 64)
    crop = T.DeviceCropper((48, 64), "cuda")
    staged = []
    crop._staging = lambda n: staged.append(n)
    occ = {"rects": [(0, 0, 4, 4)], "mode": 0, "rgb": (1, 2, 3), "seed": 1}
    for text, decision in (("radius 8", {"blur": [128] + [8] * 8}), ("= 256", {"blur": [100, 50, 27]}),
                           ("5 rectangles", {"occlusion": dict(occ, rects=[(0, 0, 4, 4)] * 5)}), ("unknown fill mode", {"occlusion": dict(occ, mode=2)})):
        with pytest.raises(_lib.PoseKernelError, match=text):
            crop(imgs, mats, flips, augment=[None] * 5 + [decision])
    with pytest.raises(_lib.PoseKernelError, match="5 augment entries for 6"):
        crop(imgs, mats, flips, augment=[{"blur": 1.0}] * 5)
    assert staged == []
