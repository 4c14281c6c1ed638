"""Numpy restatement of the device colour jitter ("Colour jitter on the device"): the yardstick pk_affine_crop_jitter_normalize
is compared to, bit for bit.

The operation is the reference's CustomColorJitter (data/examples.py:367-401) on the cropped uint8 RGB image.  The arithmetic is the
contract the kernel is written to: float32 with one rounding per operation (numpy never fuses a multiply and an add), except the crop
mean, which comes from the EXACT integer sum S of the crop's bytes:

    m = float32(float64(S) / (255 N) * float64(b)),  N = h w 3
    x = u / 255 * b;  x = (x - m) * c + m;  g = ((x0 + x1) + x2) / 3 per pixel;  x = g + (x - g) * s;  u' = trunc(clip(x, 0, 1) * 255)

The reference takes m as float32 `img.mean()` (pairwise sums) of the already scaled image: the two differ by float32 rounding of the
mean, which moves a byte by one where x * 255 lands next to an integer.  Warp and normalisation are the oracle's (oracle/warp.py).
"""
import numpy as np

from oracle import warp as ow

F = np.float32


def jitter_u8(img_u8, b, c, s):
    """(h, w, 3) uint8 RGB -> (h, w, 3) uint8, factors as the kernel receives them (float32)."""
    b, c, s = F(b), F(c), F(s)
    S = int(img_u8.astype(np.int64).sum())
    m = F(np.float64(S) / (255.0 * img_u8.size) * np.float64(b))
    x = img_u8.astype(F) / F(255.0) * b
    x = (x - m) * c + m
    g = ((x[..., 0] + x[..., 1]) + x[..., 2]) / F(3.0)
    x = g[..., None] + (x - g[..., None]) * s
    assert x.dtype == F
    return (np.minimum(np.maximum(x, F(0.0)), F(1.0)) * F(255.0)).astype(np.int32).astype(np.uint8)


def crop_jitter_normalize(img, m_fwd, out_wh, flip=False, jitter=None):
    """One sample of DeviceCropper(..., jitter=): oracle warp, jitter (None = the bypass), oracle normalisation -> (3, h, w) float32."""
    crop = ow.warp_affine_u8(img, m_fwd, out_wh, flip=flip)
    if jitter is not None:
        crop = jitter_u8(crop, *jitter)
    return ow.normalize_chw(crop)


def denormalize_to_u8(chw):
    """Normalised (3, h, w) float32 -> the (h, w, 3) bytes it was made from, through the table of the 256 x 3 values normalize_chw can
    produce (exact lookup: every entry of `chw` must be one of them)."""
    table = ow.normalize_chw(np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2))      # (3, 256, 1)
    out = np.empty(chw.shape[1:] + (3,), np.uint8)
    for ch in range(3):
        t = table[ch, :, 0]
        assert np.all(np.diff(t) > 0)
        idx = np.searchsorted(t, chw[ch])
        idx = np.minimum(idx, 255)
        assert np.array_equal(t[idx].view(np.uint32), chw[ch].view(np.uint32)), "value outside the normalisation table"
        out[..., ch] = idx
    return out
