"""Occlusion, blur and noise augmentation, host side (no GPU): the declarations of the two entries and their refusals through ctypes, the
blur weights, the numpy restatement (tests/augment_np.py) against float64 and on hand-computed cases, the statistics of the hashed noise,
the three transforms' use of the RNG stream, the unchanged default of `get_train_transforms`, the table rows `DeviceCropper` builds, and
the validators with their yaml and flag mapping."""
import argparse
import copy
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

import augment_np as anp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
SIGMAS = (0.3, 0.5, 1.0, 1.7, 2.5)


def _lib():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


def _T():
    from infantposeestimation_gaussianbias_amd.datasets import transforms as T
    return T


# ------------------------------------------------------------------------------------------------ declarations and refusals
def test_the_header_declares_the_entries_and_the_library_exports_them():
    decl = _lib().declared_symbols()
    assert decl["pk_affine_crop_augment_ws_bytes"] == ("int", [I, I, I])
    assert decl["pk_affine_crop_augment_normalize"] == ("int", [P, P, P, I, I, I, P, P, P, P, P, I64, P])
    const = _lib().CONSTANTS
    assert (const["PK_AUG_MAX_RADIUS"], const["PK_AUG_MAX_RECTS"], const["PK_AUG_ROW_BYTES"]) == (7, 4, 176)
    L = _lib().lib
    assert hasattr(L, "pk_affine_crop_augment_ws_bytes") and hasattr(L, "pk_affine_crop_augment_normalize")
    # the jitter entry's formula and its 2^32 refusal
    for n, w, h in ((64, 192, 256), (1, 2368, 2368), (3, 20, 13), (1, 7, 5)):
        assert L.pk_affine_crop_augment_ws_bytes(n, w, h) == L.pk_affine_crop_jitter_ws_bytes(n, w, h) > 0
    assert L.pk_affine_crop_augment_ws_bytes(64, 192, 256) == 4 * 64 * (192 * 256 + 192)
    for n, w, h in ((1, 2370, 2369), (0, 48, 64), (1, 0, 64), (1, 48, -1), (96, 2369, 2369)):
        assert L.pk_affine_crop_augment_ws_bytes(n, w, h) == -1 and L.pk_last_error_string().startswith(b"pk_affine_crop_augment_ws_bytes")
    assert L.pk_affine_crop_augment_ws_bytes(1, 2370, 2369) == -1 and b"2^32" in L.pk_last_error_string()


X = 0x1000          # argument checks run before anything touches the device, so a made-up non-null address is never read


def test_the_entry_refuses_bad_arguments_before_any_launch():
    L = _lib().lib
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    need = L.pk_affine_crop_augment_ws_bytes(3, 48, 64)
    ok = dict(src=X, desc=X, aug=X, n=3, w=48, h=64, o32=X, o16=X, mean=ctypes.addressof(mean), std=ctypes.addressof(mean), ws=X, ws_bytes=need)

    def go(**kw):
        a = {**ok, **kw}
        rc = L.pk_affine_crop_augment_normalize(a["src"], a["desc"], a["aug"], a["n"], a["w"], a["h"], a["o32"], a["o16"], a["mean"], a["std"],
                                                a["ws"], a["ws_bytes"], None)
        assert rc == -1, (kw, rc)
        return L.pk_last_error_string().decode()

    for k in ("src", "desc", "aug", "mean", "std", "ws"):
        assert "null pointer" in go(**{k: None, "n": 0})                      # null first, whatever else is wrong
    assert "null pointer" in go(o32=None, o16=None)                           # at least one output
    for kw in (dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(h=-3)):
        assert "bad shape" in go(**kw, ws_bytes=0)                            # the shape before the workspace
    assert "2^32" in go(w=4096, h=2048) and "exceeds 2^31" in go(n=96, w=2369, h=2369)
    assert f"{need - 1} bytes, {need} needed" in go(ws_bytes=need - 1, ws=X + 1)      # one byte short, before the alignment
    for kw in (dict(ws=X + 1), dict(ws=X + 2), dict(o16=X + 8), dict(o16=X + 2), dict(aug=X + 4), dict(aug=X + 8)):
        assert "alignment" in go(**kw), kw
    assert go(n=0).startswith("pk_affine_crop_augment_") and go(aug=X + 4).startswith("pk_affine_crop_augment_normalize:")


# ------------------------------------------------------------------------------------------------ blur weights
@pytest.mark.parametrize("sigma", SIGMAS)
def test_blur_weights(sigma):
    q = _T().blur_weights(sigma)
    R = len(q) - 1
    assert R == min(7, int(np.ceil(3 * sigma))) and 1 <= R <= 7
    assert int(q[0]) + 2 * int(q[1:].sum()) == 256
    assert np.all(np.diff(q) <= 0) and np.all(q >= 0), q                      # non-increasing from the centre
    g = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2 * sigma * sigma))
    G = g[0] + 2 * g[1:].sum()
    assert np.all(np.abs(q[1:] / 256.0 - g[1:] / G) <= 1 / 512), (q, g / G)
    assert list(q) == anp.blur_weights(sigma)                                 # the restatement's own table


def test_blur_weights_refuse_sigmas_outside_the_table():
    for bad in (0.0, -1.0, 2.51, float("nan")):
        with pytest.raises(ValueError):
            _T().blur_weights(bad)
    assert [_T().noise_amplitude(s) for s in (0.01, 2.0, 8.0, 73.0, 80.0)] == [1, 7, 28, 253, 255]
    assert [anp.noise_amplitude(s) for s in (0.01, 2.0, 8.0, 73.0, 80.0)] == [1, 7, 28, 253, 255]


# ------------------------------------------------------------------------------------------------ the restated blur
def _blur_f64(img, q):
    """Float64 convolution with the same quantised weights and clamp border, no rounding anywhere."""
    w = np.asarray(q, np.float64) / 256.0
    R = len(q) - 1
    v = img.astype(np.float64)
    for axis in (1, 0):
        n = v.shape[axis]
        acc = np.zeros_like(v)
        for k in range(-R, R + 1):
            acc += w[abs(k)] * np.take(v, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)
        v = acc
    return v


@pytest.mark.parametrize("h,w", [(13, 20), (20, 13), (5, 7), (7, 5)])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_restated_blur_is_within_one_grey_level_of_float64(h, w, sigma):
    """Each pass rounds by at most 0.5 and the weights sum to 1, so the first pass's error is not amplified: at most 1 in all."""
    img = np.random.default_rng(int(sigma * 10) + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    q = anp.blur_weights(sigma)
    got, want = anp.blur_u8(img, q), _blur_f64(img, q)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"sigma {sigma} ({h}, {w}): max |integer - float64| = {err:.4f}")
    assert err <= 1.0


@pytest.mark.parametrize("sigma", SIGMAS)
def test_restated_blur_on_a_constant_and_on_an_impulse(sigma):
    q = anp.blur_weights(sigma)
    R = len(q) - 1
    for level in (0, 1, 137, 255):
        const = np.full((9, 11, 3), level, np.uint8)
        assert np.array_equal(anp.blur_u8(const, q), const)
    img = np.zeros((17, 19, 3), np.uint8)
    img[8, 9] = 255
    got = anp.blur_u8(img, q)
    for i in range(-R, R + 1):
        for j in range(-R, R + 1):
            want = ((((255 * q[abs(i)] + 128) >> 8) * q[abs(j)] + 128) >> 8)       # horizontal offset i, then vertical offset j
            assert np.all(got[8 + j, 9 + i] == want), (i, j)
    assert got[8 + R + 1:].max() == 0 and got[:, 9 + R + 1:].max() == 0


# ------------------------------------------------------------------------------------------------ hash and noise
def test_hash_matches_a_scalar_restatement():
    def one(seed, pix, stream):
        x = (seed + pix * 0x9E3779B9 + stream * 0x85EBCA6B) % 2 ** 32
        x ^= x >> 16
        x = x * 0x7FEB352D % 2 ** 32
        x ^= x >> 15
        x = x * 0x846CA68B % 2 ** 32
        return x ^ (x >> 16)

    pix = np.array([0, 1, 2, 255, 3071, 2 ** 31, 2 ** 32 - 1])
    for seed, stream in ((0, 0), (1, 1), (2 ** 31 - 2, 0x102), (2 ** 32 - 1, 4)):
        assert [int(v) for v in anp.hash_u32(seed, pix, stream)] == [one(seed, int(p), stream) for p in pix]


def test_noise_statistics_on_a_grey_crop():
    """Grey 128, 64 x 48, amp 28: |delta| <= (28 * 510 + 256) >> 9 = 28 at the very most, so no clamp can occur."""
    h, w, amp = 48, 64, 28
    grey = np.full((h, w, 3), 128, np.uint8)
    out = anp.noise_u8(grey, amp, seed=1234)
    d = out.astype(np.int64) - 128
    assert np.array_equal(d, anp.noise_delta(h, w, amp, 1234)) and np.abs(d).max() <= 28      # nothing clamped
    N, sd = d.size, amp / (2 * np.sqrt(3))
    assert N == 9216
    print(f"noise: mean {d.mean():+.4f} (bound {4 * sd / np.sqrt(N):.4f}), std {d.std():.4f} (nominal {sd:.4f})")
    assert abs(d.mean()) <= 4 * sd / np.sqrt(N)
    assert abs(d.std() - sd) <= 0.05 * sd
    assert np.array_equal(out, anp.noise_u8(grey, amp, seed=1234))             # same seed, same field
    assert not np.array_equal(out, anp.noise_u8(grey, amp, seed=1235))         # another seed, another field
    assert not np.array_equal(d[..., 0], d[..., 1]) and not np.array_equal(d[..., 1], d[..., 2]) and not np.array_equal(d[..., 0], d[..., 2])
    # the sum of four uniform bytes: standard deviation 256 / sqrt 3 to within 1e-5 (relative)
    var4 = 4 * (256 ** 2 - 1) / 12
    assert abs(np.sqrt(var4) / (256 / np.sqrt(3)) - 1) < 1e-5
    # the clamp
    assert anp.noise_u8(np.zeros((4, 4, 3), np.uint8), 255, 7).min() == 0 and anp.noise_u8(np.full((4, 4, 3), 255, np.uint8), 255, 7).max() == 255


def test_erasing_by_hand():
    img = np.random.default_rng(2).integers(0, 256, (6, 8, 3), dtype=np.uint8)
    rects = [(1, 1, 5, 4), (3, 2, 12, 9), (-4, -4, 0, 3), (6, 0, 6, 6)]       # overlap; reaches outside; empty after clipping; empty
    out = anp.erase_u8(img, rects, [0, 1, 0, 0], [(9, 8, 7), (0, 0, 0), (1, 1, 1), (2, 2, 2)], seed=5)
    assert np.all(out[1:4, 1:3] == (9, 8, 7)) and np.all(out[1, 1:5] == (9, 8, 7))      # the part of the first the second leaves
    hh = anp.hash_u32(5, np.array([2 * 8 + 3, 5 * 8 + 7]), 2)
    assert tuple(out[2, 3]) == tuple(int(hh[0] >> s) & 255 for s in (0, 8, 16)) and tuple(out[5, 7]) == tuple(int(hh[1] >> s) & 255 for s in (0, 8, 16))
    untouched = np.ones((6, 8), bool)
    untouched[1:4, 1:5] = False
    untouched[2:6, 3:8] = False
    assert np.array_equal(out[untouched], img[untouched])


# ------------------------------------------------------------------------------------------------ the transforms
def _same_state(r1, r2):
    return np.array_equal(r1.get_state()[1], r2.get_state()[1]) and r1.get_state()[2] == r2.get_state()[2]


def test_random_blur_and_sensor_noise_draw_in_the_documented_order():
    T = _T()
    r1, r2 = np.random.RandomState(3), np.random.RandomState(3)
    tb, tn = T.RandomBlur(prob=0.5, sigma=(0.3, 2.0), rng=r1), T.SensorNoise(prob=0.5, sigma=(2.0, 10.0), rng=r1)
    on = [0, 0]
    for _ in range(200):
        d = tn(tb({}))
        want_b = None if r2.rand() > 0.5 else float(r2.uniform(0.3, 2.0))
        if r2.rand() > 0.5:
            want_n = None
        else:
            s = float(r2.uniform(2.0, 10.0))
            want_n = (s, int(r2.randint(0, 2 ** 31 - 1)))
        assert d["blur"] == want_b and d["noise"] == want_n
        on[0] += want_b is not None
        on[1] += want_n is not None
    assert 70 < on[0] < 130 and 70 < on[1] < 130 and _same_state(r1, r2)
    assert T.RandomBlur().__dict__.items() >= dict(prob=0.3, sigma=(0.3, 2.0)).items()
    assert T.SensorNoise().__dict__.items() >= dict(prob=0.3, sigma=(2.0, 10.0)).items()


def test_random_occlusion_draws_in_the_documented_order_and_records_unclipped_rectangles():
    T = _T()
    w, h = 48, 64
    r1, r2 = np.random.RandomState(4), np.random.RandomState(4)
    t = T.RandomOcclusion(prob=0.6, max_rects=3, area=(0.05, 0.4), aspect=(0.3, 3.3), fill="mean", rng=r1, input_size=(w, h))
    n_on, outside, counts = 0, 0, set()
    for _ in range(200):
        got = t({})["occlusion"]
        if r2.rand() > 0.6:
            assert got is None
            continue
        n_on += 1
        rects = []
        for _ in range(int(r2.randint(1, 4))):
            a = r2.uniform(0.05, 0.4)
            r = np.exp(r2.uniform(np.log(0.3), np.log(3.3)))
            cx, cy = r2.uniform(0, w), r2.uniform(0, h)
            sw, sh = np.sqrt(a * w * h * r), np.sqrt(a * w * h / r)
            rects.append((int(np.floor(cx - sw / 2)), int(np.floor(cy - sh / 2)), int(np.floor(cx + sw / 2)), int(np.floor(cy + sh / 2))))
        want = {"rects": rects, "mode": 0, "rgb": (124, 116, 104), "seed": int(r2.randint(0, 2 ** 31 - 1))}
        assert got == want
        counts.add(len(rects))
        outside += any(x0 < 0 or y0 < 0 or x1 > w or y1 > h for x0, y0, x1, y1 in rects)
    assert 90 < n_on < 150 and counts == {1, 2, 3} and outside > 10 and _same_state(r1, r2)       # recorded unclipped
    d = T.RandomOcclusion(rng=np.random.RandomState(0)).__dict__
    assert d.items() >= dict(prob=0.5, max_rects=2, area=(0.02, 0.2), aspect=(0.3, 3.3), fill="random", mode=1).items()
    assert T.RandomOcclusion(fill=(1, 2, 3)).rgb == (1, 2, 3) and T.RandomOcclusion(fill=(1, 2, 3)).mode == 0
    with pytest.raises(ValueError):
        T.RandomOcclusion(fill="black")
    # the seed is drawn whatever the fill: the stream does not depend on it
    ra, rb = np.random.RandomState(8), np.random.RandomState(8)
    T.RandomOcclusion(prob=1.0, fill="random", rng=ra, input_size=(w, h))({})
    T.RandomOcclusion(prob=1.0, fill=(0, 0, 0), rng=rb, input_size=(w, h))({})
    assert _same_state(ra, rb)


def _record(rng, H, W, K=17):
    x1, y1 = rng.uniform(0, W * 0.4), rng.uniform(0, H * 0.4)
    x2, y2 = x1 + rng.uniform(W * 0.3, W * 0.55), y1 + rng.uniform(H * 0.3, H * 0.55)
    return {"center": np.array([(x1 + x2) / 2, (y1 + y2) / 2], np.float32), "scale": np.array([x2 - x1, y2 - y1], np.float32) * 1.25,
            "keypoints": np.stack([rng.uniform(x1, x2, K), rng.uniform(y1, y2, K)], 1).astype(np.float32),
            "keypoints_visible": rng.choice([0.0, 1.0, 2.0], K, p=[0.2, 0.3, 0.5]).astype(np.float32), "img_width": W, "flip": False,
            "flip_pairs": [(i, i + 1) for i in range(1, 17, 2)]}


def test_train_transforms_default_is_unchanged_and_the_new_ones_come_last():
    T = _T()
    rng = np.random.default_rng(7)
    blur, noise = {"prob": 1.0, "sigma": (0.3, 2.0)}, {"prob": 1.0, "sigma": (2.0, 10.0)}
    occ = {"prob": 1.0, "max_rects": 2, "area": (0.02, 0.2), "aspect": (0.3, 3.3), "fill": "random"}
    for with_jitter in (False, True):
        kw = dict(color_jitter=(0.3, 0.3, 0.2), color_jitter_prob=1.0) if with_jitter else {}
        for i in range(10):
            rec = _record(rng, 120, 90)
            r0, r1, r2 = np.random.RandomState(50 + i), np.random.RandomState(50 + i), np.random.RandomState(50 + i)
            # today's list, built by hand from the existing classes
            hand = [T.RandomFlip(0.5, r0), T.RandomHalfBody(0.3, rng=r0), T.RandomBBoxTransform(40.0, (0.5, 1.5), rng=r0),
                    T.TopdownAffineWithRotation((48, 64))] + ([T.ColorJitter(0.3, 0.3, 0.2, prob=1.0, rng=r0)] if with_jitter else [])
            d0 = T.Compose(hand)(copy.deepcopy(rec))
            tf1 = T.get_train_transforms((48, 64), rng=r1, blur=None, noise=None, occlusion=None, **kw)
            assert [type(t) for t in tf1.transforms] == [type(t) for t in hand]
            d1 = tf1(copy.deepcopy(rec))
            assert _same_state(r0, r1) and np.array_equal(d0["matrix"], d1["matrix"]) and d0.get("jitter") == d1.get("jitter")
            assert not {"blur", "noise", "occlusion"} & set(d1)
            tf2 = T.get_train_transforms((48, 64), rng=r2, blur=blur, noise=noise, occlusion=occ, **kw)
            assert [type(t) for t in tf2.transforms] == [type(t) for t in hand] + [T.RandomBlur, T.SensorNoise, T.RandomOcclusion]
            d2 = tf2(copy.deepcopy(rec))
            assert np.array_equal(d2["matrix"], d1["matrix"]) and np.array_equal(d2["keypoints"], d1["keypoints"]) and d2.get("jitter") == d1.get("jitter")
            assert np.array_equal(d2["keypoints_visible"], d1["keypoints_visible"])                  # labels are not touched
            r1.rand()
            assert d2["blur"] == float(r1.uniform(0.3, 2.0))                                          # drawn after everything else, in this order
            r1.rand()
            assert d2["noise"] == (float(r1.uniform(2.0, 10.0)), int(r1.randint(0, 2 ** 31 - 1)))
            assert len(d2["occlusion"]["rects"]) in (1, 2) and d2["occlusion"]["mode"] == 1
    one = T.get_train_transforms((48, 64), noise=noise)
    assert [type(t) for t in one.transforms][4:] == [T.SensorNoise]


# ------------------------------------------------------------------------------------------------ the table rows
FULL = {"blur": 2.5, "noise": (8.0, 77), "occlusion": {"rects": [(2, 3, 30, 20), (10, 10, 70, 90), (-9, -9, 0, 5), (5, 40, 20, 60)],
                                                       "mode": [0, 1, 0, 1], "rgb": [(124, 116, 104), (0, 0, 0), (9, 9, 9), (1, 2, 3)], "seed": 99}}


def test_cropper_builds_the_rows_the_header_documents():
    T = _T()
    crop = T.DeviceCropper((48, 64), "cpu")
    jitter = [(1.2, 0.8, 1.1), None, None, (0.9, 1.1, 1.0)]
    augment = [None, {"blur": 0.3}, FULL, {"occlusion": {"rects": [(0, 0, 5, 5)], "mode": 0, "rgb": (1, 2, 3), "seed": 2 ** 32 - 1}, "blur": None}]
    jtab, _ = crop._jitter_table(jitter, 4)
    tab, need = crop._augment_table(augment, jtab, 4)
    assert tab.dtype.itemsize == 176 and tab.nbytes == 4 * 176 and need == _lib().lib.pk_affine_crop_augment_ws_bytes(4, 48, 64)
    for i in range(4):
        assert np.array_equal(tab[i:i + 1].view(np.uint8), anp.table_row(jitter[i], augment[i])), i
    assert tab["radius"].tolist() == [0, 1, 7, 0] and tab["amp"].tolist() == [0, 0, 28, 0] and tab["n_rects"].tolist() == [0, 0, 4, 1]
    # without jitter the jitter fields stay zero; without a decision there is no table
    tab2, _ = crop._augment_table(augment, None, 4)
    assert not tab2["jit"]["enable"].any()
    assert crop._augment_table(None, jtab, 4) == (None, 0) and crop._augment_table([None] * 4, jtab, 4) == (None, 0)
    assert crop._augment_table([None, {}, {"blur": None, "noise": None}, None], None, 4) == (None, 0)


def test_cropper_rejects_bad_decisions_before_touching_the_device():
    T, E = _T(), _lib().PoseKernelError
    img, m = np.zeros((20, 20, 3), np.uint8), np.array([[1., 0, 0], [0, 1., 0]])
    crop = T.DeviceCropper((12, 16), "cpu")
    staged = []
    crop._staging = lambda n: staged.append(n)          # raising comes before anything is staged
    occ = {"rects": [(0, 0, 4, 4)], "mode": 0, "rgb": (1, 2, 3), "seed": 1}
    bad = [("radius", {"blur": [128] + [8] * 8}),                               # R = 8
           ("= 256", {"blur": [100, 50, 27]}),                                  # sums to 254
           ("weights", {"blur": [258, -1]}), ("sigma", {"blur": 2.6}), ("sigma", {"blur": 0.0}),
           ("5 rectangles", {"occlusion": dict(occ, rects=[(0, 0, 4, 4)] * 5)}),
           ("mode", {"occlusion": dict(occ, mode=2)}), ("mode", {"occlusion": dict(occ, mode="random")}),
           ("rgb", {"occlusion": dict(occ, rgb=(1, 2, 256))}), ("bounds", {"occlusion": dict(occ, rects=[(0, 0, 4.5, 4)])}),
           ("bounds", {"occlusion": dict(occ, rects=[(0, 0, 2 ** 31, 4)])}), ("seed", {"occlusion": dict(occ, seed=-1)}),
           ("occlusion must be", {"occlusion": {"rects": []}}), ("noise", {"noise": (0.0, 1)}), ("noise", {"noise": (3.0, 2 ** 32)}),
           ("noise", {"noise": 3.0}), ("keys", {"erase": 1}), ("keys", [1, 2])]
    for text, decision in bad:
        with pytest.raises(E, match=f"augment 1.*{text}"):
            crop([img, img], [m, m], augment=[None, decision])
    with pytest.raises(E, match="1 augment entries for 2"):
        crop([img, img], [m, m], augment=[{"blur": 1.0}])
    with pytest.raises(E, match="2\\^32"):
        T.DeviceCropper((4096, 2048), "cpu")([img], [m], augment=[{"blur": 1.0}])
    assert staged == []


# ------------------------------------------------------------------------------------------------ validators, yaml, flags
def test_check_augment_refuses_each_bad_value_with_its_key():
    from infantposeestimation_gaussianbias_amd.configs.config import AUGMENT_DEFAULTS, check_augment
    assert check_augment("blur", None) is None and check_augment("blur", {}) is None and check_augment("noise", {"prob": 0}) is None
    assert check_augment("blur", {"prob": 0.5}) == {"prob": 0.5, "sigma": (0.3, 2.0)}
    assert check_augment("noise", {"sigma": [1, 73]}) == {"prob": 0.3, "sigma": (1.0, 73.0)}
    assert check_augment("occlusion", {"fill": [1, 2, 3], "max_rects": 4}) == dict(AUGMENT_DEFAULTS["occlusion"], fill=(1, 2, 3), max_rects=4)
    assert check_augment("occlusion", {"fill": "mean"})["fill"] == "mean"
    bad = [("blur", {"prob": 1.5}, "prob"), ("blur", {"prob": -0.1}, "prob"), ("blur", {"prob": "x"}, "prob"),
           ("blur", {"sigma": (0.0, 1.0)}, "sigma"), ("blur", {"sigma": (1.0, 0.5)}, "sigma"), ("blur", {"sigma": (0.3, 2.6)}, "sigma"),
           ("blur", {"sigma": 1.0}, "sigma"), ("noise", {"sigma": (2.0, 73.5)}, "sigma"), ("noise", {"sigma": (0, 5)}, "sigma"),
           ("occlusion", {"max_rects": 0}, "max_rects"), ("occlusion", {"max_rects": 5}, "max_rects"), ("occlusion", {"max_rects": 1.5}, "max_rects"),
           ("occlusion", {"area": (0.0, 0.2)}, "area"), ("occlusion", {"area": (0.2, 1.2)}, "area"), ("occlusion", {"area": (0.3, 0.2)}, "area"),
           ("occlusion", {"aspect": (0.0, 2.0)}, "aspect"), ("occlusion", {"aspect": (3.0, 2.0)}, "aspect"),
           ("occlusion", {"fill": "black"}, "fill"), ("occlusion", {"fill": (1, 2)}, "fill"), ("occlusion", {"fill": (1, 2, 300)}, "fill"),
           ("occlusion", {"colour": 1}, "keys")]
    for kind, setting, key in bad:
        with pytest.raises(ValueError, match=f"FLAG.*{key}"):
            check_augment(kind, setting, "FLAG")
    # what the validator returns is what the transforms take
    T = _T()
    T.get_train_transforms((48, 64), blur=check_augment("blur", {"prob": 0.5}), noise=check_augment("noise", {"prob": 0.5}),
                           occlusion=check_augment("occlusion", {"prob": 0.5}))


def test_config_carries_the_settings_outside_the_dataclass_surface(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import config as C
    from infantposeestimation_gaussianbias_amd.configs import get_config
    cfg = get_config()
    names = {f.name for f in dataclasses.fields(C.TrainConfig)}
    for attr in ("blur", "sensor_noise", "occlusion"):
        assert getattr(cfg.train, attr) is None and attr not in names and attr not in dataclasses.asdict(cfg)["train"]
    cfg.train.blur = {"prob": 0.3, "sigma": (0.3, 2.0)}
    assert dataclasses.asdict(cfg) == dataclasses.asdict(get_config()) and get_config().train.blur is None      # per instance
    y = tmp_path / "with.yaml"
    y.write_text("MODEL:\n  NUM_JOINTS: 13\nDATA:\n  BLUR:\n    PROB: 0.4\n    SIGMA: [0.5, 1.5]\n  NOISE:\n    SIGMA: [1, 20]\n"
                 "  OCCLUSION:\n    PROB: 0.7\n    MAX_RECTS: 3\n    AREA: [0.05, 0.3]\n    ASPECT: [0.5, 2]\n    FILL: mean\n")
    got = get_config(str(y))
    assert got.train.blur == {"prob": 0.4, "sigma": (0.5, 1.5)} and got.train.sensor_noise == {"prob": 0.3, "sigma": (1.0, 20.0)}
    assert got.train.occlusion == {"prob": 0.7, "max_rects": 3, "area": (0.05, 0.3), "aspect": (0.5, 2.0), "fill": "mean"}
    assert got.data.num_keypoints == 13 and got.train.color_jitter is None
    y2 = tmp_path / "rgb.yaml"
    y2.write_text("DATA:\n  OCCLUSION:\n    FILL: [10, 20, 30]\n")
    assert get_config(str(y2)).train.occlusion["fill"] == (10, 20, 30) and get_config(str(y2)).train.occlusion["prob"] == 0.5
    for k, text in enumerate(("DATA:\n  BLUR: {}\n  NOISE: {}\n  OCCLUSION: {}\n", "DATA:\n  BLUR:\n    PROB: 0\n  NOISE:\n    PROB: 0.0\n    SIGMA: [1, 2]\n"
                              "  OCCLUSION:\n    PROB: 0\n", "MODEL:\n  SIGMA: 1.5\nDATA:\n  FLIP: true\n")):
        y0 = tmp_path / f"off{k}.yaml"
        y0.write_text(text)
        t = get_config(str(y0)).train
        assert t.blur is None and t.sensor_noise is None and t.occlusion is None
    for key, text in (("DATA.BLUR", "DATA:\n  BLUR:\n    SIGMA: [0.3, 3.0]\n"), ("DATA.NOISE", "DATA:\n  NOISE:\n    PROB: 2\n"),
                      ("DATA.OCCLUSION", "DATA:\n  OCCLUSION:\n    MAX_RECTS: 5\n"), ("DATA.OCCLUSION", "DATA:\n  OCCLUSION:\n    FILL: black\n"),
                      ("DATA.BLUR", "DATA:\n  BLUR: 3\n")):
        yb = tmp_path / "bad.yaml"
        yb.write_text(text)
        with pytest.raises(ValueError, match=key):
            get_config(str(yb))


def _train():
    import importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("train")


def test_train_flags_set_the_same_attributes():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    train = _train()
    p = train.build_parser()

    def cfg_of(argv, cfg=None):
        cfg = cfg or get_config()
        train.apply_augment_flags(cfg, p.parse_args(argv))
        return cfg.train

    t = cfg_of([])
    assert t.blur is None and t.sensor_noise is None and t.occlusion is None
    t = cfg_of(["--blur", "0.4", "1.5", "--noise", "0.2", "12", "--occlusion", "0.6", "3"])
    assert t.blur == {"prob": 0.4, "sigma": (0.3, 1.5)} and t.sensor_noise == {"prob": 0.2, "sigma": (2.0, 12.0)}
    assert t.occlusion == {"prob": 0.6, "max_rects": 3, "area": (0.02, 0.2), "aspect": (0.3, 3.3), "fill": "random"}
    assert cfg_of(["--blur", "0.4", "0.2"]).blur == {"prob": 0.4, "sigma": (0.2, 0.2)}          # below the default's lower end
    t = cfg_of(["--occlusion", "0.6", "1", "--occlusion_area", "0.1", "0.5", "--occlusion_fill", "mean"])
    assert t.occlusion["area"] == (0.1, 0.5) and t.occlusion["fill"] == "mean" and t.occlusion["max_rects"] == 1
    assert cfg_of(["--occlusion", "1", "2", "--occlusion_fill", "10,20,30"]).occlusion["fill"] == (10, 20, 30)
    t = cfg_of(["--blur", "0", "2.0", "--noise", "0", "5", "--occlusion", "0", "2"])           # PROB 0: off
    assert t.blur is None and t.sensor_noise is None and t.occlusion is None
    # a flag goes over what a yaml set
    base = get_config()
    base.train.blur, base.train.occlusion = {"prob": 0.9, "sigma": (1.0, 2.0)}, {"prob": 0.9, "max_rects": 4, "area": (0.1, 0.2), "aspect": (1.0, 2.0), "fill": "mean"}
    t = cfg_of(["--blur", "0", "1", "--occlusion", "0.5", "2"], base)
    assert t.blur is None and t.occlusion == {"prob": 0.5, "max_rects": 2, "area": (0.1, 0.2), "aspect": (1.0, 2.0), "fill": "mean"}
    for argv, flag in ((["--blur", "0.5", "3.0"], "--blur"), (["--blur", "1.5", "1.0"], "--blur"), (["--noise", "0.5", "80"], "--noise"),
                       (["--noise", "0.5", "0"], "--noise"), (["--occlusion", "0.5", "5"], "--occlusion"), (["--occlusion", "0.5", "1.5"], "--occlusion"),
                       (["--occlusion", "0.5", "2", "--occlusion_area", "0.5", "0.1"], "--occlusion_area"),
                       (["--occlusion", "0.5", "2", "--occlusion_fill", "black"], "--occlusion_fill"),
                       (["--occlusion", "0.5", "2", "--occlusion_fill", "1,2"], "--occlusion_fill"),
                       (["--occlusion_fill", "mean"], "--occlusion_fill"), (["--occlusion_area", "0.1", "0.2"], "--occlusion_area")):
        with pytest.raises(ValueError, match=flag):
            cfg_of(argv)
    assert isinstance(p, argparse.ArgumentParser)
