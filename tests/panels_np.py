"""numpy restatement of the feature-sheet and heat-map-quality entries, written from the text of include/posekernels.h
(pk_gather_planes, pk_plane_sheet_size, pk_plane_sheet, pk_heatmap_quality) and of utils/visualization.colour_ramp.

The colour index is computed with np.float32 scalars-as-arrays in the stated order (numpy rounds every float32 operation once, as the
kernel does without FMA); the records in float64, the sums in the stated order (per thread ascending, xor butterfly, waves left to right),
so that they can be compared bit for bit as well as within the a-priori bound of a float64 sum."""
import numpy as np

THREADS, WAVE = 256, 64
F32 = np.float32


# ------------------------------------------------------------------------------------------------ ramps
def _piecewise(anchors):
    t = np.arange(256, dtype=np.float64) / 255.0
    a = np.asarray(anchors, np.float64)
    pos = np.linspace(0.0, 1.0, len(a))
    rgb = np.stack([np.interp(t, pos, a[:, c]) for c in range(3)], axis=1)
    return np.rint(rgb).astype(np.uint8)[:, ::-1]


def colour_ramp(name):
    t = np.arange(256, dtype=np.float64) / 255.0
    clip = lambda v: np.clip(v, 0.0, 1.0)      # noqa: E731
    if name == "hot":
        rgb = np.stack([clip(t / 0.365079), clip((t - 0.365079) / 0.380953), clip((t - 0.746032) / 0.253968)], axis=1)
        return np.rint(255.0 * rgb).astype(np.uint8)[:, ::-1]
    if name == "sequential":
        return _piecewise([(68, 1, 84), (59, 82, 139), (33, 145, 140), (94, 201, 98), (253, 231, 37)])
    if name == "diverging":
        return _piecewise([(59, 76, 192), (221, 221, 221), (180, 4, 38)])
    if name == "jet":
        chan = lambda c: np.rint(255.0 * clip(1.5 - np.abs(4.0 * t - c))).astype(np.uint8)      # noqa: E731
        return np.stack([chan(1.0), chan(2.0), chan(3.0)], axis=1)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ planes
def gather_planes(x_f32, b, channels, c_used):
    """x_f32: (B,H,W,C) float32 holding the bf16 values exactly."""
    _, H, W, _ = x_f32.shape
    out = np.full((len(channels), H, W), np.nan, np.float32)
    for i, c in enumerate(channels):
        if 0 <= c < c_used:
            out[i] = x_f32[b, :, :, c]
    return out


# ------------------------------------------------------------------------------------------------ the sheet
def sheet_size(T, h, w, cols, zoom, pad):
    rows = -(-T // cols)
    return pad + rows * (h * zoom + pad), pad + cols * (w * zoom + pad)


def tile_index(v):
    """(h,w) float32 -> (idx (h,w) int, lo, hi) by the header's rule."""
    v = np.asarray(v, F32)
    fin = np.isfinite(v)
    lo = F32(v[fin].min()) if fin.any() else F32(np.inf)
    hi = F32(v[fin].max()) if fin.any() else F32(-np.inf)
    with np.errstate(all="ignore"):
        den = F32(F32(hi - lo) + F32(1e-8))
        u = ((v - lo).astype(F32) / den).astype(F32)
        f = np.floor((F32(255.0) * u).astype(F32))
    idx = np.where(f >= 255.0, 255, np.where(f > 0.0, f, 0.0))         # a NaN fails both comparisons: 0
    idx = np.where(fin, np.nan_to_num(idx, nan=0.0), 0.0).astype(np.int64)
    return idx, lo, hi


def plane_sheet(a, b, tiles, luts, cols, zoom, pad, bg):
    a = np.asarray(a, F32)
    Na, h, w = a.shape
    Nb = 0 if b is None else b.shape[0]
    luts = np.asarray(luts, np.uint8).reshape(-1, 256, 3)
    T = len(tiles)
    SH, SW = sheet_size(T, h, w, cols, zoom, pad)
    sheet = np.empty((SH, SW, 3), np.uint8)
    sheet[:] = np.asarray(bg, np.uint8)
    ranges = np.empty((T, 2), F32)
    for t, (ia, ib, ramp) in enumerate(tiles):
        if not (0 <= ia < Na and ib < Nb and 0 <= ramp < len(luts)):
            ranges[t] = np.nan
            continue
        with np.errstate(all="ignore"):
            v = a[ia] if ib < 0 else np.abs((a[ia] - np.asarray(b, F32)[ib]).astype(F32))
        idx, lo, hi = tile_index(v)
        ranges[t] = lo, hi
        y0, x0 = pad + (t // cols) * (h * zoom + pad), pad + (t % cols) * (w * zoom + pad)
        big = np.repeat(np.repeat(idx, zoom, axis=0), zoom, axis=1)
        sheet[y0:y0 + h * zoom, x0:x0 + w * zoom] = luts[ramp][big]
    return sheet, ranges


# ------------------------------------------------------------------------------------------------ heat-map quality
def ordered_sum(terms):
    """The header's order: thread r adds terms r, r + 256, ... in ascending order to 0.0, the xor butterfly 32 .. 1 inside each wave, then
    wave 0 + wave 1 + wave 2 + wave 3.  `terms` = (values, mask): 1-D float64 values, one per element of the map, and the elements that
    take part; a thread skips the others, so they add nothing (not even a +0.0)."""
    vals, mask = terms
    n = len(vals)
    acc = np.zeros(THREADS, np.float64)
    for k in range(0, n, THREADS):
        chunk, keep = vals[k:k + THREADS], mask[k:k + THREADS]
        m = len(chunk)
        acc[:m] = np.where(keep, acc[:m] + chunk, acc[:m])
    lanes = acc.reshape(THREADS // WAVE, WAVE)
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(WAVE) ^ o]
        o >>= 1
    total = lanes[0, 0]
    for wv in range(1, THREADS // WAVE):
        total = total + lanes[wv, 0]
    return total


def _peak(v, ok, w):
    """First of equal maxima in row-major order among the counted elements; -inf at (0, 0) without a value above -inf."""
    cand = np.where(ok, v, -np.inf)
    if not (cand > -np.inf).any():
        return -np.inf, 0.0, 0.0
    i = int(np.argmax(cand))                                           # numpy's argmax returns the first of equal maxima
    return float(v[i]), float(i % w), float(i // w)


def heatmap_quality(pred, gt):
    """(M,h,w) float32 x2 -> (records (M,16) float64, abs_terms (M,16) float64: the sum of |terms| behind each summed column)."""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    M, h, w = pred.shape
    rec, mag = np.zeros((M, 16), np.float64), np.zeros((M, 16), np.float64)
    for m in range(M):
        p32, g32 = pred[m].reshape(-1), gt[m].reshape(-1)
        ok = np.isfinite(p32) & np.isfinite(g32)
        with np.errstate(all="ignore"):
            p, g = np.where(ok, p32, 0).astype(np.float64), np.where(ok, g32, 0).astype(np.float64)
        n = int(ok.sum())
        d = p - g
        r = rec[m]
        r[0], r[1], r[2] = ordered_sum((p, ok)), ordered_sum((g, ok)), ordered_sum((d * d, ok))
        mag[m, 0], mag[m, 1], mag[m, 2] = np.abs(p[ok]).sum(), np.abs(g[ok]).sum(), (d * d)[ok].sum()
        r[3] = np.abs(d[ok]).max() if n else 0.0
        r[4:7] = _peak(p32, ok, w)
        r[7:10] = _peak(g32, ok, w)
        with np.errstate(all="ignore"):
            mp, mg = r[0] / np.float64(n), r[1] / np.float64(n)
            dp, dg = p - mp, g - mg
        r[10], r[11], r[12] = ordered_sum((dp * dg, ok)), ordered_sum((dp * dp, ok)), ordered_sum((dg * dg, ok))
        if n:
            mag[m, 10], mag[m, 11], mag[m, 12] = np.abs(dp * dg)[ok].sum(), (dp * dp)[ok].sum(), (dg * dg)[ok].sum()
        if r[4] > 0 and r[7] > 0:
            in_p = ok & (p32 >= F32(0.5) * F32(r[4]))
            in_g = ok & (g32 >= F32(0.5) * F32(r[7]))
            r[13], r[14] = (in_p & in_g).sum(), (in_p | in_g).sum()
        r[15] = p32.size - n
    return rec, mag
