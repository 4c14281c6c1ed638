"""Data augmentation / crop transforms (drop-in names for the reference's datasets/transforms.py), split for the MI355X pipeline:

  * the per-sample DECISIONS and the 17-keypoint arithmetic (flip, half-body, scale / rotation draws, the affine matrix, keypoint
    transform and visibility) stay on the host -- a few dozen flops per sample, same numpy expressions and the same order of
    `np.random` draws as the reference, so a seeded run consumes the RNG stream identically;
  * the image work (affine crop, mirror, BGR->RGB, ToTensor, normalise) is NOT done per sample with OpenCV: the transforms only record
    `data['matrix']` / `data['flip']`, and `DeviceCropper` warps the whole batch in one kernel (pk_affine_crop_normalize) straight into
    the network's input layout.  At ~3 000 img/s per GPU the reference's 4 DataLoader workers doing cv2.warpAffine would be ~7x too slow.
    Photometric augmentation follows the same split: `ColorJitter` only draws the factors (`data['jitter']`), the crop's launch
    sequence applies them (pk_affine_crop_jitter_normalize).  So do `RandomBlur`, `SensorNoise` and `RandomOcclusion` (soft focus,
    low-light noise, blankets and cables over the limbs): they record `data['blur']` / `data['noise']` / `data['occlusion']`, and
    pk_affine_crop_augment_normalize blurs, adds noise and erases on the device.  Labels never change.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import call, stream_ptr

MEAN = np.array([0.485, 0.456, 0.406], np.float32)      # datasets/coco_dataset.py:160-161
STD = np.array([0.229, 0.224, 0.225], np.float32)


class Compose:
    def __init__(self, transforms: List):
        self.transforms = transforms

    def __call__(self, data: Dict) -> Dict:
        for t in self.transforms:
            data = t(data)
        return data


def _get_dir(src_point, rot_rad):
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    return np.array([src_point[0] * cs - src_point[1] * sn, src_point[0] * sn + src_point[1] * cs])


def _get_3rd_point(a, b):
    direct = a - b
    return b + np.array([-direct[1], direct[0]], dtype=np.float32)


def get_affine_matrix(center, scale, output_size, rot: float = 0.0) -> np.ndarray:
    """transforms.py:58-88: the 2x3 float64 matrix cv2.getAffineTransform returns for the three point pairs (6x6 solve)."""
    src_w, dst_w, dst_h = scale[0], output_size[0], output_size[1]
    src_dir = _get_dir([0, src_w * -0.5], np.pi * rot / 180)
    dst_dir = np.array([0, dst_w * -0.5], np.float32)
    src, dst = np.zeros((3, 2), dtype=np.float32), np.zeros((3, 2), dtype=np.float32)
    src[0, :], src[1, :] = center, center + src_dir
    dst[0, :] = [dst_w * 0.5, dst_h * 0.5]
    dst[1, :] = np.array([dst_w * 0.5, dst_h * 0.5]) + dst_dir
    src[2, :], dst[2, :] = _get_3rd_point(src[0, :], src[1, :]), _get_3rd_point(dst[0, :], dst[1, :])
    a, b = np.zeros((6, 6)), np.zeros(6)
    for i in range(3):
        a[i, 0:2], a[i, 2], a[i + 3, 3:5], a[i + 3, 5] = src[i], 1.0, src[i], 1.0
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def multiscale_matrices(center, scale, scales, input_size) -> List[np.ndarray]:
    """The crop matrices of a multi-scale test: per entry s of `scales` the un-rotated crop of box scale `scale * s` around the same
    centre.  An input pixel u of the scale-1.0 crop lies at W/2 + (u - W/2) / s in the scale-s crop (what pk_multiscale_merge undoes)."""
    scale = np.asarray(scale)
    return [get_affine_matrix(center, scale * s, input_size, 0) for s in scales]


def invert_affine(m) -> np.ndarray:
    """Destination -> source matrix exactly as cv::warpAffine derives it (float64)."""
    m = np.asarray(m, np.float64).copy().reshape(6)
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0], m[1], m[3], m[4] = a11, m[1] * -d, m[3] * -d, a22
    b1, b2 = -m[0] * m[2] - m[1] * m[5], -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


class TopdownAffine:
    """Records the crop matrix and applies it to the visible keypoints (transforms.py:22-56); the image is warped later, on the device."""

    def __init__(self, input_size: Tuple[int, int]):
        self.input_size = np.array(input_size)

    def _matrix(self, data):
        return get_affine_matrix(data['center'], data['scale'], self.input_size, 0)

    def __call__(self, data: Dict) -> Dict:
        trans = self._matrix(data)
        kp = data['keypoints']
        for i in range(len(kp)):
            if data['keypoints_visible'][i] > 0:
                kp[i] = np.dot(trans, np.array([kp[i][0], kp[i][1], 1.]).T)[:2]
        data['matrix'], data['keypoints'] = trans, kp
        return data


class TopdownAffineWithRotation(TopdownAffine):
    """transforms.py:196-232: + rotation; a visible keypoint that leaves the crop becomes invisible."""

    def _matrix(self, data):
        return get_affine_matrix(data['center'], data['scale'], self.input_size, data.get('rotation', 0))

    def __call__(self, data: Dict) -> Dict:
        trans = self._matrix(data)
        kp, vis = data['keypoints'], data['keypoints_visible']
        for i in range(len(kp)):
            if vis[i] > 0:
                kp[i] = np.dot(trans, np.array([kp[i][0], kp[i][1], 1.]).T)[:2]
                if kp[i, 0] < 0 or kp[i, 0] >= self.input_size[0] or kp[i, 1] < 0 or kp[i, 1] >= self.input_size[1]:
                    vis[i] = 0
        data['matrix'], data['keypoints'] = trans, kp
        return data


class RandomFlip:
    """transforms.py:108-150; the image itself is mirrored by the crop kernel (`data['flip']`)."""

    def __init__(self, flip_prob: float = 0.5, rng=None):
        self.flip_prob, self.rng = flip_prob, rng or np.random

    def __call__(self, data: Dict) -> Dict:
        if self.rng.random() < self.flip_prob:
            w = data['img_width']
            data['center'][0] = w - data['center'][0] - 1
            kp, vis = data['keypoints'], data['keypoints_visible']
            kp[:, 0] = w - kp[:, 0] - 1
            for a, b in data.get('flip_pairs', []):
                kp[a], kp[b] = kp[b].copy(), kp[a].copy()
                vis[a], vis[b] = vis[b], vis[a]
            data['flip'] = not data.get('flip', False)
        return data


class RandomBBoxTransform:
    """transforms.py:153-193."""

    def __init__(self, rotation_factor: float = 40.0, scale_factor: Tuple[float, float] = (0.5, 1.5), rotation_prob: float = 0.6, rng=None):
        self.rotation_factor, self.scale_factor, self.rotation_prob, self.rng = rotation_factor, scale_factor, rotation_prob, rng or np.random

    def __call__(self, data: Dict) -> Dict:
        data['scale'] = data['scale'] * self.rng.uniform(self.scale_factor[0], self.scale_factor[1])
        if self.rng.random() < self.rotation_prob:
            data['rotation'] = np.clip(self.rng.randn() * self.rotation_factor, -self.rotation_factor * 2, self.rotation_factor * 2)
        else:
            data['rotation'] = 0
        return data


class RandomHalfBody:
    """transforms.py:235-290."""
    UPPER_BODY_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    LOWER_BODY_IDS = [11, 12, 13, 14, 15, 16]

    def __init__(self, prob: float = 0.3, min_keypoints: int = 3, rng=None):
        self.prob, self.min_keypoints, self.rng = prob, min_keypoints, rng or np.random

    def __call__(self, data: Dict) -> Dict:
        if self.rng.random() > self.prob:
            return data
        kp, vis = data['keypoints'], data['keypoints_visible']
        upper = [kp[i] for i in self.UPPER_BODY_IDS if i < len(vis) and vis[i] > 0]
        lower = [kp[i] for i in self.LOWER_BODY_IDS if i < len(vis) and vis[i] > 0]
        if len(upper) >= self.min_keypoints and len(lower) >= self.min_keypoints:
            sel = upper if self.rng.random() < 0.5 else lower
        elif len(upper) >= self.min_keypoints:
            sel = upper
        elif len(lower) >= self.min_keypoints:
            sel = lower
        else:
            return data
        sel = np.array(sel)
        lo, hi = sel.min(axis=0), sel.max(axis=0)
        data['center'] = sel.mean(axis=0)
        data['scale'] = np.maximum(np.array([hi[0] - lo[0], hi[1] - lo[1]]) * 1.5, data['scale'] * 0.5)
        return data


class ColorJitter:
    """The decisions of the reference's CustomColorJitter (data/examples.py:367-401): the same draws in the same order -- `rand()`,
    and unless it is above `prob`, `uniform` for brightness, contrast and saturation.  Records `data['jitter'] = (b, c, s)` or None;
    the image is jittered by the crop's launch sequence on the device (`DeviceCropper(..., jitter=)`)."""

    def __init__(self, brightness: float = 0.2, contrast: float = 0.2, saturation: float = 0.2, prob: float = 0.5, rng=None):
        self.brightness, self.contrast, self.saturation, self.prob, self.rng = brightness, contrast, saturation, prob, rng or np.random

    def __call__(self, data: Dict) -> Dict:
        data['jitter'] = None
        if self.rng.rand() > self.prob:
            return data
        data['jitter'] = tuple(1 + self.rng.uniform(-r, r) for r in (self.brightness, self.contrast, self.saturation))
        return data


MEAN_FILL = (124, 116, 104)      # the ImageNet mean in bytes: round(255 * MEAN)
SEED_HIGH = 2 ** 31 - 1          # seeds are drawn with randint(0, SEED_HIGH)


def blur_weights(sigma) -> np.ndarray:
    """The integer taps q[0 .. R] (centre, then one side) of the device blur for 0 < sigma <= 2.5, in float64: R = min(7, ceil(3 sigma)),
    g_k = exp(-k^2 / (2 sigma^2)), G = g_0 + 2 sum_{k>=1} g_k, sides q_k = rint(256 g_k / G) (half to even), centre q_0 = 256 - 2 sum q_k,
    so that q_0 + 2 sum q_k = 256 exactly.  The device evaluates no exp: it gets this table."""
    sigma = float(sigma)
    if not 0 < sigma <= 2.5:
        raise ValueError(f"blur sigma must be in (0, 2.5], got {sigma!r}")
    R = min(7, int(np.ceil(3.0 * sigma)))
    g = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    G = g[0] + 2.0 * g[1:].sum()
    q = np.rint(256.0 * g / G).astype(np.int32)
    q[0] = 256 - 2 * int(q[1:].sum())
    return q


def noise_amplitude(sigma) -> int:
    """The integer amplitude of the device noise for a standard deviation of `sigma` grey levels: the added value is (amp s + 256) >> 9
    with s a sum of four uniform bytes less 510 (standard deviation 256 / sqrt 3), i.e. amp / (2 sqrt 3) grey levels."""
    return int(min(255, max(1, np.rint(2.0 * np.sqrt(3.0) * float(sigma)))))


class RandomBlur:
    """Decides the Gaussian blur of the crop: `rand()`, and unless it is above `prob`, `uniform(lo, hi)` for sigma.  Records
    `data['blur'] = sigma` or None; the crop's launch sequence blurs on the device (`DeviceCropper(..., augment=)`)."""

    def __init__(self, prob: float = 0.3, sigma: Tuple[float, float] = (0.3, 2.0), rng=None):
        self.prob, self.sigma, self.rng = prob, tuple(sigma), rng or np.random

    def __call__(self, data: Dict) -> Dict:
        data['blur'] = None
        if self.rng.rand() > self.prob:
            return data
        data['blur'] = float(self.rng.uniform(self.sigma[0], self.sigma[1]))
        return data


class SensorNoise:
    """Decides the additive sensor noise: `rand()`, and unless it is above `prob`, `uniform(lo, hi)` for sigma (grey levels) and
    `randint(0, 2**31 - 1)` for the seed of the device hash.  Records `data['noise'] = (sigma, seed)` or None."""

    def __init__(self, prob: float = 0.3, sigma: Tuple[float, float] = (2.0, 10.0), rng=None):
        self.prob, self.sigma, self.rng = prob, tuple(sigma), rng or np.random

    def __call__(self, data: Dict) -> Dict:
        data['noise'] = None
        if self.rng.rand() > self.prob:
            return data
        sigma = float(self.rng.uniform(self.sigma[0], self.sigma[1]))
        data['noise'] = (sigma, int(self.rng.randint(0, SEED_HIGH)))
        return data


class RandomOcclusion:
    """Decides the erased rectangles of the crop (blankets, cables, hands over the limbs).  Draws, in this order: `rand()`; unless it is
    above `prob`, `n = randint(1, max_rects + 1)`; per rectangle the area fraction `a = uniform(area)`, the aspect ratio
    `r = exp(uniform(log aspect_lo, log aspect_hi))` and the centre `cx = uniform(0, w)`, `cy = uniform(0, h)`; then the seed
    `randint(0, 2**31 - 1)`, whatever the fill.  No retries.  A rectangle is sqrt(a w h r) wide and sqrt(a w h / r) high, its integer bounds
    floor(c -+ side / 2) are recorded UNCLIPPED (the device clips).  `fill`: 'random' (hashed bytes), 'mean' (the ImageNet mean bytes) or
    an (r, g, b) byte triple.  Records `data['occlusion'] = {'rects': [(x0, y0, x1, y1), ...], 'mode': 0 | 1, 'rgb': (r, g, b), 'seed'}`
    or None.  Labels are not touched: learning to place an occluded joint is the point.  (w, h) is `input_size`, the crop's size."""

    def __init__(self, prob: float = 0.5, max_rects: int = 2, area: Tuple[float, float] = (0.02, 0.2), aspect: Tuple[float, float] = (0.3, 3.3),
                 fill='random', rng=None, input_size=None):
        self.prob, self.max_rects, self.area, self.aspect, self.rng = prob, int(max_rects), tuple(area), tuple(aspect), rng or np.random
        self.fill, self.input_size = fill, input_size
        if isinstance(fill, str) and fill not in ('random', 'mean'):
            raise ValueError(f"RandomOcclusion: fill must be 'random', 'mean' or an (r, g, b) byte triple, got {fill!r}")
        self.mode = 1 if fill == 'random' else 0
        self.rgb = (0, 0, 0) if fill == 'random' else MEAN_FILL if fill == 'mean' else tuple(int(v) for v in fill)

    def __call__(self, data: Dict) -> Dict:
        data['occlusion'] = None
        if self.rng.rand() > self.prob:
            return data
        size = self.input_size if self.input_size is not None else data['input_size']
        w, h = int(size[0]), int(size[1])
        rects = []
        for _ in range(int(self.rng.randint(1, self.max_rects + 1))):
            a = self.rng.uniform(self.area[0], self.area[1])
            r = np.exp(self.rng.uniform(np.log(self.aspect[0]), np.log(self.aspect[1])))
            cx, cy = self.rng.uniform(0, w), self.rng.uniform(0, h)
            sw, sh = np.sqrt(a * w * h * r), np.sqrt(a * w * h / r)
            rects.append((int(np.floor(cx - sw / 2)), int(np.floor(cy - sh / 2)), int(np.floor(cx + sw / 2)), int(np.floor(cy + sh / 2))))
        data['occlusion'] = {'rects': rects, 'mode': self.mode, 'rgb': self.rgb, 'seed': int(self.rng.randint(0, SEED_HIGH))}
        return data


def get_train_transforms(input_size, flip_prob=0.5, rotation_factor=40.0, scale_factor=(0.5, 1.5), rng=None, color_jitter=None,
                         color_jitter_prob=0.5, blur=None, noise=None, occlusion=None) -> Compose:
    """`color_jitter`: None (no photometric augmentation, no extra draws) or the (brightness, contrast, saturation) ranges.  `blur`,
    `noise`, `occlusion`: None (off, no extra draws) or the keyword dict of `RandomBlur` / `SensorNoise` / `RandomOcclusion` (what
    `configs.config.check_augment` returns); the configured ones come after `ColorJitter`, in that order."""
    tf = [RandomFlip(flip_prob, rng), RandomHalfBody(0.3, rng=rng), RandomBBoxTransform(rotation_factor, scale_factor, rng=rng),
          TopdownAffineWithRotation(input_size)]
    if color_jitter is not None:
        tf.append(ColorJitter(*color_jitter, prob=color_jitter_prob, rng=rng))
    if blur is not None:
        tf.append(RandomBlur(**blur, rng=rng))
    if noise is not None:
        tf.append(SensorNoise(**noise, rng=rng))
    if occlusion is not None:
        tf.append(RandomOcclusion(**occlusion, rng=rng, input_size=tuple(input_size)))
    return Compose(tf)


def get_val_transforms(input_size) -> Compose:
    return Compose([TopdownAffine(input_size)])


_CROP_DTYPE = np.dtype([("off", "<i8"), ("H", "<i4"), ("W", "<i4"), ("flip", "<i4"), ("bgr", "<i4"), ("minv", "<f8", (6,))])
_JITTER_DTYPE = np.dtype([("enable", "<i4"), ("b", "<f4"), ("c", "<f4"), ("s", "<f4")])
# one aug_table row of pk_affine_crop_augment_normalize (posekernels.h)
MAX_RADIUS, MAX_RECTS = _lib.CONSTANTS["PK_AUG_MAX_RADIUS"], _lib.CONSTANTS["PK_AUG_MAX_RECTS"]
_AUG_RECT_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("mode", "<i4"), ("rgb", "<u4")])
_AUG_DTYPE = np.dtype([("jit", _JITTER_DTYPE), ("radius", "<i4"), ("q", "<i4", (MAX_RADIUS + 1,)), ("amp", "<i4"), ("noise_seed", "<u4"),
                       ("n_rects", "<i4"), ("erase_seed", "<u4"), ("rect", _AUG_RECT_DTYPE, (MAX_RECTS,)), ("pad", "<i4", (3,))])
assert _AUG_DTYPE.itemsize == _lib.CONSTANTS["PK_AUG_ROW_BYTES"]


def _is_int(v, lo, hi):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) and lo <= int(v) <= hi


def augment_row(tab, i, decision):
    """Fill row `i` of the aug_table `tab` (_AUG_DTYPE; the jitter fields are the caller's) from that crop's decision: a dict with any of
      'blur': sigma in (0, 2.5] (-> `blur_weights`), or the integer taps q[0 .. R] themselves (R = 1 .. 7, q >= 0, q[0] + 2 sum q[1:] = 256);
      'noise': (sigma, seed), sigma > 0 in grey levels (-> `noise_amplitude`), 0 <= seed < 2^32;
      'occlusion': {'rects': up to 4 (x0, y0, x1, y1) integer bounds, 'mode': 0 (constant) | 1 (random), 'rgb': (r, g, b) bytes, 'seed'};
                   'mode' and 'rgb' may also be lists with one entry per rectangle.
    A key that is missing or None leaves its stage off.  PoseKernelError naming crop `i` for anything else."""
    def bad(msg):
        return _lib.PoseKernelError(f"DeviceCropper: augment {i}: {msg}")

    if not isinstance(decision, dict) or set(decision) - {"blur", "noise", "occlusion"}:
        raise bad(f"must be None or a dict with keys from 'blur', 'noise', 'occlusion', got {decision!r}")
    blur, noise, occ = decision.get("blur"), decision.get("noise"), decision.get("occlusion")
    if blur is not None:
        if np.ndim(blur) == 0:
            try:
                q = blur_weights(blur)
            except (TypeError, ValueError) as e:
                raise bad(str(e)) from None
        else:
            q = list(blur)
            if not 2 <= len(q) <= MAX_RADIUS + 1:
                raise bad(f"blur radius {len(q) - 1} outside 1 .. {MAX_RADIUS}")
            if not all(_is_int(v, 0, 256) for v in q):
                raise bad(f"blur weights must be integers in 0 .. 256, got {q!r}")
            if int(q[0]) + 2 * sum(int(v) for v in q[1:]) != 256:
                raise bad(f"blur weights must satisfy q[0] + 2 sum(q[1:]) = 256, got {q!r}")
        tab["radius"][i] = len(q) - 1
        tab["q"][i, :len(q)] = q
    if noise is not None:
        try:
            sigma, seed = noise
            ok = np.isfinite(float(sigma)) and float(sigma) > 0 and _is_int(seed, 0, 2 ** 32 - 1)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise bad(f"noise must be (sigma > 0, 0 <= seed < 2^32), got {noise!r}")
        tab["amp"][i], tab["noise_seed"][i] = noise_amplitude(sigma), int(seed)
    if occ is not None:
        if not isinstance(occ, dict) or set(occ) != {"rects", "mode", "rgb", "seed"}:
            raise bad(f"occlusion must be a dict with 'rects', 'mode', 'rgb' and 'seed', got {occ!r}")
        n = len(occ["rects"])
        if n > MAX_RECTS:
            raise bad(f"{n} rectangles (at most {MAX_RECTS})")
        if not _is_int(occ["seed"], 0, 2 ** 32 - 1):
            raise bad(f"occlusion seed must be an integer in [0, 2^32), got {occ['seed']!r}")
        tab["n_rects"][i], tab["erase_seed"][i] = n, int(occ["seed"])
        if n == 0:
            return
        # whole arrays at once (this runs per sample and per step): integer dtypes only, so 4.5, True or 'random' do not pass
        try:
            rc, mode, rgb = np.asarray(occ["rects"]), np.asarray(occ["mode"]), np.asarray(occ["rgb"])
        except ValueError:            # ragged lists
            raise bad(f"occlusion rects / mode / rgb must be rectangular lists of integers, got {occ!r}") from None
        if rc.shape != (n, 4) or rc.dtype.kind not in "iu" or rc.min() < -2 ** 31 or rc.max() > 2 ** 31 - 1:
            raise bad(f"rectangles must be four int32 bounds (x0, y0, x1, y1) each, got {occ['rects']!r}")
        if mode.shape not in ((), (n,)) or mode.dtype.kind not in "iu" or mode.min() < 0 or mode.max() > 1:
            raise bad(f"unknown fill mode in {occ['mode']!r} (0 = constant, 1 = random; one, or one per rectangle)")
        if rgb.shape not in ((3,), (n, 3)) or rgb.dtype.kind not in "iu" or rgb.min() < 0 or rgb.max() > 255:
            raise bad(f"rgb must be three bytes (one triple, or one per rectangle), got {occ['rgb']!r}")
        rows = tab["rect"][i, :n]
        rows["x0"], rows["y0"], rows["x1"], rows["y1"], rows["mode"] = rc[:, 0], rc[:, 1], rc[:, 2], rc[:, 3], mode
        rgb = rgb.astype(np.uint32)
        rows["rgb"] = rgb[..., 0] | rgb[..., 1] << 8 | rgb[..., 2] << 16


class DeviceCropper:
    """Batched affine crop + mirror + normalise on the GPU.  `images`: list of (H,W,3) uint8 arrays (numpy or torch, host);
    `matrices`: the forward 2x3 crop matrices; `jitter`: per image None or the (b, c, s) factors of `ColorJitter`;
    -> (fp32 NCHW batch | None, bf16 NHWC-8 batch | None).  The work goes to the current stream; the scratch of the jitter launches is
    kept per stream, so one cropper may serve several streams.  That cache is never pruned: one allocation (12.6 MB at B = 64, 256 x 192)
    stays for every stream the cropper has ever been called on -- sized for the project's one or two streams, not for a cropper shared by
    many short-lived ones."""

    def __init__(self, input_size, device="cuda", nchw=True, nhwc8=True):
        self.w, self.h, self.device, self.nchw, self.nhwc8 = int(input_size[0]), int(input_size[1]), torch.device(device), nchw, nhwc8
        # two reusable pinned staging buffers (pin_memory() per batch is a hipHostMalloc of ~15 MB each time); a slot is rewritten only
        # after the host-to-device copy that last read it has completed (its event)
        self._pinned, self._pin_ev, self._slot = [None, None], [None, None], 0
        self._jitter_ws = {}        # workspace of the jitter launches per stream, kept between calls: calls on one stream are ordered, a
                                    # second stream must not overwrite the crop scratch the first one's second launch still reads

    def _staging(self, nbytes):
        if not torch.cuda.is_available():
            return torch.empty(nbytes, dtype=torch.uint8), None
        i = self._slot = self._slot ^ 1
        if self._pin_ev[i] is not None:
            self._pin_ev[i].synchronize()
        if self._pinned[i] is None or self._pinned[i].numel() < nbytes:
            self._pinned[i] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return self._pinned[i][:nbytes], i

    def _jitter_table(self, jitter, B):
        """-> (table, workspace bytes), or (None, 0) when no sample is jittered (the plain call)."""
        if jitter is None:
            return None, 0
        if len(jitter) != B:
            raise _lib.PoseKernelError(f"DeviceCropper: {len(jitter)} jitter entries for {B} images")
        if all(j is None for j in jitter):
            return None, 0
        tab = np.zeros(B, _JITTER_DTYPE)
        for i, j in enumerate(jitter):
            if j is not None:
                if len(j) != 3 or not np.all(np.isfinite(np.asarray(j, np.float32))):
                    raise _lib.PoseKernelError(f"DeviceCropper: jitter {i} must be three finite factors (b, c, s), got {j!r}")
                tab[i] = (1, j[0], j[1], j[2])
        need = _lib.lib.pk_affine_crop_jitter_ws_bytes(B, self.w, self.h)
        if need <= 0:
            raise _lib.PoseKernelError(_lib.lib.pk_last_error_string().decode())
        return tab, need

    def _augment_table(self, augment, jtab, B):
        """-> (table, workspace bytes), or (None, 0) when no crop carries a blur, noise or occlusion decision (the plain or the jitter
        call).  `jtab`: the jitter table of `_jitter_table` or None; its rows become the jitter fields of this table's."""
        if augment is None:
            return None, 0
        if len(augment) != B:
            raise _lib.PoseKernelError(f"DeviceCropper: {len(augment)} augment entries for {B} images")
        if all(a is None or (isinstance(a, dict) and all(v is None for v in a.values())) for a in augment):
            return None, 0
        tab = np.zeros(B, _AUG_DTYPE)
        if jtab is not None:
            tab["jit"] = jtab
        for i, a in enumerate(augment):
            if a is not None:
                augment_row(tab, i, a)
        need = _lib.lib.pk_affine_crop_augment_ws_bytes(B, self.w, self.h)
        if need <= 0:
            raise _lib.PoseKernelError(_lib.lib.pk_last_error_string().decode())
        return tab, need

    def __call__(self, images, matrices, flips=None, bgr=False, jitter=None, image_index=None, augment=None):
        """`image_index` (one entry per crop): crop i reads images[image_index[i]], so several crops (the persons of one frame) share
        one staged and uploaded image; `matrices`, `flips` and `jitter` then have one entry per crop.  Without it crop i reads image i.
        `augment` (one entry per crop): None or the crop's blur / noise / occlusion decisions as `augment_row` takes them (the values
        `RandomBlur`, `SensorNoise` and `RandomOcclusion` record).  With at least one decision the batch goes through
        pk_affine_crop_augment_normalize (jitter included); without any, through exactly the call it would take without the keyword."""
        if image_index is None:
            src_of = range(len(images))
        else:
            src_of = [int(j) for j in image_index]
            if any(j < 0 or j >= len(images) for j in src_of):
                raise _lib.PoseKernelError(f"DeviceCropper: image_index entries must be in [0, {len(images)}), got {src_of}")
        B = len(src_of)
        if B == 0 or len(matrices) != B:
            raise _lib.PoseKernelError("DeviceCropper: need one matrix per image" if image_index is None else
                                       f"DeviceCropper: {len(matrices)} matrices for {B} image_index entries")
        if image_index is not None and flips is not None and len(flips) != B:
            raise _lib.PoseKernelError(f"DeviceCropper: {len(flips)} flips for {B} image_index entries")
        jtab, ws_bytes = self._jitter_table(jitter, B)
        atab, aug_ws_bytes = self._augment_table(augment, jtab, B)
        entry = "pk_affine_crop_jitter_normalize"
        if atab is not None:          # the augmentation table takes the jitter table's place (its rows carry the jitter fields)
            jtab, ws_bytes, entry = atab, aug_ws_bytes, "pk_affine_crop_augment_normalize"
        sizes, offs, off = [], [], 0
        for i, im in enumerate(images):
            im = im.numpy() if torch.is_tensor(im) else np.asarray(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise _lib.PoseKernelError(f"DeviceCropper: image {i} must be (H,W,3) uint8, got {im.dtype} {im.shape}")
            sizes.append(im)
            offs.append(off)
            off += (im.size + 15) // 16 * 16
        desc = np.zeros(B, _CROP_DTYPE)
        for i, j in enumerate(src_of):
            desc[i] = (offs[j], sizes[j].shape[0], sizes[j].shape[1], int(bool(flips[i])) if flips is not None else 0, int(bool(bgr)),
                       invert_affine(matrices[i]))
        nd, nj = desc.nbytes, 0 if jtab is None else jtab.nbytes
        joff = off + (nd + 15) // 16 * 16
        host, slot = self._staging(joff + (nj + 15) // 16 * 16)         # [images | descriptor table | jitter or augmentation table]: ONE copy
        # plain memcpy through a numpy view: a torch slice assignment fans every 0.9 MB image out over all intra-op threads (128 on the
        # GPU host: 21 ms per 64 images against 1.4 ms; scripts/probes/cropper_phases.py)
        hv = host.numpy()
        for o, im in zip(offs, sizes):
            np.copyto(hv[o:o + im.size], np.ascontiguousarray(im).reshape(-1))
        np.copyto(hv[off:off + nd], desc.view(np.uint8))
        if nj:
            np.copyto(hv[joff:joff + nj], jtab.view(np.uint8))
        dev_buf = host.to(self.device, non_blocking=True)
        if slot is not None:
            self._pin_ev[slot] = torch.cuda.Event()
            self._pin_ev[slot].record()
        src, dtab = dev_buf[:off], dev_buf[off:off + nd]
        out32 = torch.empty(B, 3, self.h, self.w, dtype=torch.float32, device=self.device) if self.nchw else None
        out16 = torch.empty(B, self.h, self.w, 8, dtype=torch.bfloat16, device=self.device) if self.nhwc8 else None
        if jtab is None:
            call("pk_affine_crop_normalize", src, dtab, B, self.w, self.h, out32, out16, MEAN.ctypes.data, STD.ctypes.data, stream_ptr())
        else:
            st = stream_ptr()
            ws = self._jitter_ws.get(st)
            if ws is None or ws.numel() < ws_bytes:
                ws = self._jitter_ws[st] = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            call(entry, src, dtab, dev_buf[joff:joff + nj], B, self.w, self.h, out32, out16, MEAN.ctypes.data, STD.ctypes.data, ws, ws.numel(), st)
        dev_buf.record_stream(torch.cuda.current_stream())
        return out32, out16
