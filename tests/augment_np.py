"""Numpy restatement of the device augmentation ("Occlusion, blur and noise on the device"): the yardstick
pk_affine_crop_augment_normalize is compared to, bit for bit.  Stages 3 to 5 -- blur, noise, erasing -- are integer arithmetic on the
(h, w, 3) uint8 crop; the warp and the normalisation are the oracle's (oracle/warp.py), the jitter is tests/jitter_np.py.

    hash(seed, pix, stream): x = seed + pix 0x9E3779B9 + stream 0x85EBCA6B; x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B;
                             x ^= x >> 16                                     (uint32, mod 2^32; pix = y w + x)
    blur:    t = (sum_k q[|k|] u(clamp(x + k), y) + 128) >> 8, then v = (sum_k q[|k|] t(x, clamp(y + k)) + 128) >> 8
    noise:   s = sum of the four bytes of hash(noise_seed, pix, 0x100 + c) - 510;  v' = clamp(v + ((amp s + 256) >> 9), 0, 255)
    erasing: rectangle r, mode 0: its RGB bytes; mode 1: bytes 0, 1, 2 of hash(erase_seed, pix, 1 + r); later over earlier

Nothing here imports the package: the weights, the amplitude and the table rows are restated as well.
"""
import numpy as np

import jitter_np
from oracle import warp as ow

MAX_RADIUS, MAX_RECTS, ROW_BYTES = 7, 4, 176
MEAN_FILL = (124, 116, 104)


def blur_weights(sigma):
    """q[0 .. R] for 0 < sigma <= 2.5, float64: R = min(7, ceil(3 sigma)); sides rint(256 g_k / G); centre 256 - 2 sum of the sides."""
    R = min(7, int(np.ceil(3.0 * np.float64(sigma))))
    g = [np.exp(-np.float64(k * k) / (2.0 * np.float64(sigma) ** 2)) for k in range(R + 1)]
    G = g[0] + 2.0 * sum(g[1:])
    side = [int(np.rint(256.0 * gk / G)) for gk in g[1:]]
    return [256 - 2 * sum(side)] + side


def noise_amplitude(sigma):
    return int(min(255, max(1, np.rint(2.0 * np.sqrt(3.0) * sigma))))


def hash_u32(seed, pix, stream):
    """`pix` any integer array; -> uint32 array."""
    M = np.uint64(0xFFFFFFFF)
    x = (np.uint64(seed) + np.asarray(pix, np.uint64) * np.uint64(0x9E3779B9) + np.uint64(stream) * np.uint64(0x85EBCA6B)) & M
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def _pass(u, q, axis):
    """One blur pass of an int64 (h, w, 3) image along `axis` (0: vertical, 1: horizontal), clamp-to-edge."""
    R, n = len(q) - 1, u.shape[axis]
    acc = np.zeros_like(u)
    for k in range(-R, R + 1):
        idx = np.clip(np.arange(n) + k, 0, n - 1)
        acc += int(q[abs(k)]) * np.take(u, idx, axis=axis)
    return (acc + 128) >> 8


def blur_u8(img, q):
    """(h, w, 3) uint8 -> uint8; q = [centre, side 1, ..., side R] with q[0] + 2 sum(q[1:]) = 256."""
    assert int(q[0]) + 2 * sum(int(v) for v in q[1:]) == 256 and 1 <= len(q) - 1 <= MAX_RADIUS
    v = _pass(_pass(img.astype(np.int64), q, 1), q, 0)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def noise_delta(h, w, amp, seed):
    """The (h, w, 3) int64 values the noise stage adds before its clamp."""
    pix = np.arange(h * w, dtype=np.int64).reshape(h, w)
    out = np.empty((h, w, 3), np.int64)
    for c in range(3):
        hh = hash_u32(seed, pix, 0x100 + c).astype(np.int64)
        s = (hh & 255) + ((hh >> 8) & 255) + ((hh >> 16) & 255) + (hh >> 24) - 510
        out[..., c] = (amp * s + 256) >> 9          # numpy's >> on a signed integer floors, like the device's arithmetic shift
    return out


def noise_u8(img, amp, seed):
    h, w, _ = img.shape
    return np.clip(img.astype(np.int64) + noise_delta(h, w, amp, seed), 0, 255).astype(np.uint8)


def erase_u8(img, rects, modes, rgbs, seed):
    """`rects`: (x0, y0, x1, y1), unclipped; modes / rgbs: one per rectangle."""
    h, w, _ = img.shape
    out = img.copy()
    pix = np.arange(h * w, dtype=np.int64).reshape(h, w)
    for r, ((x0, y0, x1, y1), mode, rgb) in enumerate(zip(rects, modes, rgbs)):
        xa, xb, ya, yb = max(x0, 0), min(x1, w), max(y0, 0), min(y1, h)
        if xa >= xb or ya >= yb:
            continue
        if mode == 0:
            out[ya:yb, xa:xb] = np.asarray(rgb, np.uint8)
        else:
            hh = hash_u32(seed, pix[ya:yb, xa:xb], 1 + r)
            for c in range(3):
                out[ya:yb, xa:xb, c] = ((hh >> np.uint32(8 * c)) & np.uint32(255)).astype(np.uint8)
    return out


def _per_rect(occ):
    n = len(occ["rects"])
    modes = list(occ["mode"]) if np.ndim(occ["mode"]) else [occ["mode"]] * n
    rgbs = list(occ["rgb"]) if np.ndim(occ["rgb"]) == 2 else [occ["rgb"]] * n
    return modes, rgbs


def augment_u8(crop, jitter=None, decision=None):
    """Stages 2 to 5 on a warped (h, w, 3) uint8 crop.  `decision`: None or {'blur': sigma | weights, 'noise': (sigma, seed),
    'occlusion': {'rects', 'mode', 'rgb', 'seed'}} as DeviceCropper takes it."""
    d = decision or {}
    if jitter is not None:
        crop = jitter_np.jitter_u8(crop, *jitter)
    if d.get("blur") is not None:
        crop = blur_u8(crop, blur_weights(d["blur"]) if np.ndim(d["blur"]) == 0 else list(d["blur"]))
    if d.get("noise") is not None:
        crop = noise_u8(crop, noise_amplitude(d["noise"][0]), d["noise"][1])
    if d.get("occlusion") is not None:
        occ = d["occlusion"]
        crop = erase_u8(crop, occ["rects"], *_per_rect(occ), occ["seed"])
    return crop


def crop_augment_normalize(img, m_fwd, out_wh, flip=False, jitter=None, decision=None):
    """One sample of DeviceCropper(..., jitter=, augment=): oracle warp, stages 2 to 5, oracle normalisation -> (3, h, w) float32."""
    return ow.normalize_chw(augment_u8(ow.warp_affine_u8(img, m_fwd, out_wh, flip=flip), jitter, decision))


def table_row(jitter=None, decision=None):
    """The 176 bytes of one aug_table row as posekernels.h lays them out."""
    d = decision or {}
    i4, u4, f4 = "<i4", "<u4", "<f4"
    parts = [np.array([0 if jitter is None else 1], i4), np.array(jitter if jitter is not None else (0, 0, 0), f4)]
    q = [] if d.get("blur") is None else (blur_weights(d["blur"]) if np.ndim(d["blur"]) == 0 else list(d["blur"]))
    parts += [np.array([max(len(q) - 1, 0)], i4), np.array(list(q) + [0] * (8 - len(q)), i4)]
    amp, nseed = (0, 0) if d.get("noise") is None else (noise_amplitude(d["noise"][0]), d["noise"][1])
    parts += [np.array([amp], i4), np.array([nseed], u4)]
    occ = d.get("occlusion")
    rects = [] if occ is None else list(occ["rects"])
    parts += [np.array([len(rects)], i4), np.array([0 if occ is None else occ["seed"]], u4)]
    modes, rgbs = ([], []) if occ is None else _per_rect(occ)
    for r in range(MAX_RECTS):
        if r < len(rects):
            parts += [np.array(list(rects[r]) + [modes[r]], i4), np.array([rgbs[r][0] | rgbs[r][1] << 8 | rgbs[r][2] << 16], u4)]
        else:
            parts += [np.zeros(5, i4), np.zeros(1, u4)]
    parts.append(np.zeros(3, i4))
    row = np.concatenate([p.view(np.uint8) for p in parts])
    assert row.size == ROW_BYTES
    return row
