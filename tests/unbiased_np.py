"""numpy restatement of pk_unbiased_decode (include/posekernels.h), independent of the kernel's patch form: the WHOLE zero-padded map is
blurred separably (row pass, then column pass, taps ascending), its logarithm taken, and the same derivative formulas applied at the
first maximum.  It runs in float32 (every operation rounded once; the fused multiply-adds through an exact float64 product) or in float64
(the taps are the same float32 values either way), and returns the coordinates, the `refined` flag and the margin of every condition of
the step, so a test can tell a decision that hangs on the last bits from one that does not.

Also here: the taps by their formula, the input generator of the unbiased-decode tests (Gaussian peaks of amplitude 1 at uniform sub-pixel
centres plus N(0, noise^2) per pixel, seeded) and numpy forms of pk_argmax_decode's modes 1 and 2 for the accuracy comparison."""
import numpy as np

CLAMP = 1e-10
# Margin below which a condition of the step counts as undecided between float32 and float64.  The float32 log map differs from the
# float64 one by the blur's rounding (at most ksize + 1 <= 32 roundings of 2^-24 relative on B, i.e. <= 2e-6 absolute on L where the sum
# does not cancel) plus logf's own error (a few 2^-24 |L|, |L| <= 23.1: <= 5e-6), together below 1e-5.  A second difference is a quarter of
# four such terms (<= 1e-5) and det a difference of two products of them with factors below 1 (<= 6e-5): for `dxx` and `det` 1e-3 is at
# least 16 times what float32 can move the margin.  The offsets are quotients by det, so no such bound holds for `ox` / `oy` in general;
# there the margin rests on the conditioning the tests assert before they compare anything (the float32 and the float64 restatement
# agree within 1e-5 px on every map), of which 1e-3 is a hundred times.
MARGIN = 1e-3


def taps(k):
    """float32 taps by the formula of hipops.unbiased_taps, written out independently."""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    c = (k - 1) // 2
    g = np.array([np.exp(-((i - c) ** 2) / (2.0 * sigma * sigma)) for i in range(k)], np.float64)
    return (g / g.sum()).astype(np.float32)


def _fma(g, v, acc, dtype):
    if dtype == np.float64:
        return g * v + acc
    return (g.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)      # exact product, then one (double) rounding


def blur(maps, g, dtype):
    """(N, H, W) -> B (N, H, W): zero padding, row pass then column pass, acc = fma(g[t], m[.. + t - c], acc) for t ascending."""
    g = np.asarray(g, np.float32).astype(dtype)
    k, c = g.size, (g.size - 1) // 2
    m = np.asarray(maps).astype(dtype)
    N, H, W = m.shape
    pad = np.zeros((N, H, W + 2 * c), dtype)
    pad[:, :, c:c + W] = m
    R = np.zeros((N, H, W), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(k):
            R = _fma(g[t], pad[:, :, t:t + W], R, dtype)
        pad = np.zeros((N, H + 2 * c, W), dtype)
        pad[:, c:c + H, :] = R
        B = np.zeros((N, H, W), dtype)
        for t in range(k):
            B = _fma(g[t], pad[:, t:t + H, :], B, dtype)
    return B


def first_max(maps):
    """torch.max / am_block: NaN counts as the maximum, ties go to the lowest flat index -> (index (N,) int64, value (N,) float32)."""
    flat = np.asarray(maps, np.float32).reshape(len(maps), -1)
    idx = np.empty(len(flat), np.int64)
    for n, row in enumerate(flat):
        nan = np.isnan(row)
        idx[n] = int(np.argmax(nan)) if nan.any() else int(np.argmax(row))
    return idx, flat[np.arange(len(flat)), idx]


def decode(maps, g, dtype=np.float64):
    """maps (N, H, W) float32, g the float32 taps -> dict: index (N,) int64, maxval (N,) float32, coords (N, 2) `dtype`, refined (N,) uint8,
    interior (N,) bool, offsets (N, 2) and margins {'dxx': -dxx, 'det': det, 'ox': 2 - |ox|, 'oy': 2 - |oy|} (each (N,), positive = the
    condition holds; NaN where the map is not interior)."""
    dtype = np.dtype(dtype).type
    maps = np.asarray(maps, np.float32)
    N, H, W = maps.shape
    idx, mv = first_max(maps)
    px, py = idx % W, idx // W
    interior = (px >= 2) & (px <= W - 3) & (py >= 2) & (py <= H - 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = np.log(np.fmax(blur(maps, g, dtype), dtype(CLAMP)))          # fmax like fmaxf: a NaN sum reads as the clamp
    coords = np.stack([px, py], 1).astype(dtype)
    refined = np.zeros(N, np.uint8)
    off = np.full((N, 2), np.nan, dtype)
    margins = {k: np.full(N, np.nan, np.float64) for k in ("dxx", "det", "ox", "oy")}
    h, q, two = dtype(0.5), dtype(0.25), dtype(2.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for n in np.nonzero(interior)[0]:
            l, x, y = L[n], int(px[n]), int(py[n])
            dx = h * (l[y, x + 1] - l[y, x - 1])
            dy = h * (l[y + 1, x] - l[y - 1, x])
            dxx = q * (l[y, x + 2] - two * l[y, x] + l[y, x - 2])
            dyy = q * (l[y + 2, x] - two * l[y, x] + l[y - 2, x])
            dxy = q * (l[y + 1, x + 1] - l[y - 1, x + 1] - l[y + 1, x - 1] + l[y - 1, x - 1])
            det = dxx * dyy - dxy * dxy
            ox = -((dyy * dx - dxy * dy) / det)
            oy = -((dxx * dy - dxy * dx) / det)
            margins["dxx"][n], margins["det"][n], margins["ox"][n], margins["oy"][n] = -dxx, det, 2.0 - abs(ox), 2.0 - abs(oy)
            off[n] = ox, oy
            if dxx < 0 and det > 0 and abs(ox) <= 2 and abs(oy) <= 2:
                refined[n] = 1
                coords[n] = dtype(x) + ox, dtype(y) + oy
    return {"index": idx, "maxval": mv, "coords": coords, "refined": refined, "interior": interior, "offsets": off, "margins": margins}


def decided(res, margin=MARGIN):
    """(N,) bool: the step's decision does not hang on the last bits.  True where the peak is not interior (an integer test), where some
    condition fails by more than `margin` or is NaN (a NaN fails in every precision) in the order the conditions are written, or where
    all four hold by more than `margin`."""
    m = res["margins"]
    out = ~res["interior"]
    for n in np.nonzero(res["interior"])[0]:
        v = [m[k][n] for k in ("dxx", "det", "ox", "oy")]
        if all(x > margin for x in v):
            out[n] = True
            continue
        for x in v:                       # the first condition that does not clearly hold decides
            if x > margin:
                continue
            out[n] = bool(np.isnan(x) or x < -margin)
            break
    return out


# ------------------------------------------------------------------------------------------------ inputs
def make_maps(n, H, W, seed, sigmas=(1.5, 2.0), noise=0.02, border=4.0):
    """n maps (n, H, W) float32 and their true centres (n, 2) float64 (x, y): a Gaussian peak of amplitude 1, sigma drawn from `sigmas`,
    centre uniform in [border, W - 1 - border] x [border, H - 1 - border], plus N(0, noise^2) per pixel."""
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(border, W - 1 - border, n), rng.uniform(border, H - 1 - border, n)
    sg = rng.choice(np.asarray(sigmas, np.float64), n)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    maps = np.exp(-((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2) / (2 * sg[:, None, None] ** 2))
    maps = maps + rng.normal(0.0, noise, maps.shape) if noise > 0 else maps
    return maps.astype(np.float32), np.stack([cx, cy], 1)


def peak_at(H, W, cx, cy, sigma=1.5):
    """One noise-free map (H, W) float32 with its peak centred at (cx, cy)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma ** 2)).astype(np.float32)


def mean_error(coords, centres):
    return float(np.sqrt(((np.asarray(coords, np.float64) - centres) ** 2).sum(1)).mean())


# ------------------------------------------------------------------------------------------------ pk_argmax_decode modes 1 and 2
def decode_shift(maps):
    """Mode 1: argmax plus a quarter pixel toward the larger neighbour (1 <= p <= size - 2)."""
    maps = np.asarray(maps, np.float32)
    N, H, W = maps.shape
    idx, _ = first_max(maps)
    out = np.stack([idx % W, idx // W], 1).astype(np.float32)
    for n in range(N):
        x, y, m = int(idx[n] % W), int(idx[n] // W), maps[n]
        if 0 < x < W - 1 and 0 < y < H - 1:
            out[n, 0] += np.float32(0.25) * np.sign(m[y, x + 1] - m[y, x - 1])
            out[n, 1] += np.float32(0.25) * np.sign(m[y + 1, x] - m[y - 1, x])
    return out


def decode_taylor(maps):
    """Mode 2: the per-axis Taylor step on the raw map, clamped to half a pixel (1 < p < size - 1, second difference negative)."""
    maps = np.asarray(maps, np.float32)
    N, H, W = maps.shape
    idx, _ = first_max(maps)
    out = np.stack([idx % W, idx // W], 1).astype(np.float32)
    f = np.float32
    for n in range(N):
        x, y, m = int(idx[n] % W), int(idx[n] // W), maps[n]
        if 1 < x < W - 1 and 1 < y < H - 1:
            c, l, r, u, d = m[y, x], m[y, x - 1], m[y, x + 1], m[y - 1, x], m[y + 1, x]
            dxx, dyy = (r - f(2) * c) + l, (d - f(2) * c) + u
            if dxx < 0:
                out[n, 0] += np.clip((r - l) / (f(2) * abs(dxx)), f(-0.5), f(0.5))
            if dyy < 0:
                out[n, 1] += np.clip((d - u) / (f(2) * abs(dyy)), f(-0.5), f(0.5))
    return out
