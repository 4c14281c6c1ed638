"""numpy restatement of pk_multiscale_merge (include/posekernels.h), operation for operation in float32.

The kernel's fmaf rounds once; numpy has no fused multiply-add, so it is emulated as float32(float64(a) * float64(b) + float64(c)): the
product of two float32 is exact in float64, the sum is rounded to float64 and then to float32 (a double rounding that can differ from the
fused result by one float32 ulp in rare ties; the GPU test's tolerance carries it)."""
import numpy as np

F32 = np.float32


def fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def lerp(a, b, t):
    return fmaf(t, (b - a).astype(F32), a)


def inv_scales(scales):
    """float32(1.0 / float64(scale)) per entry: the table the op layer hands to the entry point."""
    return (1.0 / np.asarray(scales, np.float64)).astype(F32)


def sample_coords(n, inv):
    """Pass coordinate of the n base pixels 0 .. n-1 along one axis: fmaf(u - n/2, inv, n/2), float32."""
    c = F32(0.5) * F32(n)
    return fmaf(np.arange(n, dtype=F32) - c, F32(inv), c)


def merge(stack, scales, B, partner=None, flip=False):
    """stack (S*F*B, K, H, W) float32 pass-major (pass s*F + f) -> (B, K, H, W) float32."""
    stack = np.asarray(stack)
    assert stack.dtype == F32 and stack.ndim == 4
    S, F = len(scales), 2 if flip else 1
    N, K, H, W = stack.shape
    assert N == S * F * B and (not flip or len(partner) == K)
    inv = inv_scales(scales)
    acc = np.zeros((B, K, H, W), F32)
    cnt = np.zeros((H, W), np.int32)
    for s in range(S):
        us, vs = sample_coords(W, inv[s]), sample_coords(H, inv[s])
        okx, oky = (us >= 0) & (us <= F32(W - 1)), (vs >= 0) & (vs <= F32(H - 1))
        inside = oky[:, None] & okx[None, :]                       # (H, W)
        ux, vy = np.where(okx, us, F32(0)), np.where(oky, vs, F32(0))   # outside samples are computed on a dummy tap and discarded
        x0, y0 = np.floor(ux).astype(np.int64), np.floor(vy).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        lx = np.broadcast_to((ux - x0.astype(F32)).astype(F32)[None, :], (H, W))
        ly = np.broadcast_to((vy - y0.astype(F32)).astype(F32)[:, None], (H, W))
        for f in range(F):
            m = stack[(s * F + f) * B:(s * F + f + 1) * B]
            if f == 1:
                m = m[:, np.asarray(partner, np.int64)]
            c0, c1 = (W - 1 - x0, W - 1 - x1) if f == 1 else (x0, x1)
            top = lerp(m[:, :, y0[:, None], c0[None, :]], m[:, :, y0[:, None], c1[None, :]], lx)
            bot = lerp(m[:, :, y1[:, None], c0[None, :]], m[:, :, y1[:, None], c1[None, :]], lx)
            val = lerp(top, bot, ly)
            acc = np.where(inside, (acc + val).astype(F32), acc)
            cnt = cnt + inside.astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (acc / cnt.astype(F32)).astype(F32)
    return np.where(cnt > 0, out, F32(0)).astype(F32)


def border_margins(n, scales):
    """The inside / outside decision along an axis of n pixels, in exact rational arithmetic (a scale is the decimal it was written as):
    for every scale and base pixel the distance of the exact sample coordinate n/2 + (u - n/2) / s from the nearer border (0 or n-1), and
    whether the float32 arithmetic lands on that exact value (a sample ON a border is then decided alike everywhere).
    -> per scale (distances float64 (n,), exact bool (n,))."""
    from fractions import Fraction
    out = []
    for s, inv in zip(scales, inv_scales(scales)):
        fs, got = Fraction(float(s)).limit_denominator(10000), sample_coords(n, inv)
        e = [Fraction(n, 2) + (u - Fraction(n, 2)) / fs for u in range(n)]
        dist = np.array([float(min(abs(v), abs(v - (n - 1)))) for v in e])
        out.append((dist, np.array([Fraction(float(g)) == v for g, v in zip(got, e)])))
    return out


def assert_borders_are_decided_alike(shape_hw, scales, margin=1e-3):
    """No sample coordinate of these shapes lies within `margin` px of a border of its pass unless it is exactly on it with exact float32
    arithmetic: kernel and restatement cannot then disagree about which passes see a pixel."""
    for n in shape_hw:
        for s, (dist, exact) in zip(scales, border_margins(n, scales)):
            bad = (dist < margin) & ~((dist == 0) & exact)
            assert not bad.any(), f"axis of {n} px, scale {s}: base pixels {np.nonzero(bad)[0].tolist()} sample within {margin} px of a border"


# ---- shared by the host and the device tests
PARTNER = [0, 2, 1]          # one self-partner, one pair
EPS = 2.0 ** -24


def tolerance(stack, S, F):
    """|out - ref| <= 32 S F 2^-24 max|stack|: <= 3 lerps of 2 roundings per sample, S F accumulations, one division, the double rounding of
    the emulated fma, and a coordinate rounding of 2^-24 W px against a slope of at most 2 max|stack| per px.  Derived, not measured."""
    return 32 * S * F * EPS * float(np.abs(stack).max())


def ramp_stack(scales, B, K, H, W, flip, partner=PARTNER):
    """Pass s holds g(cx + (x - cx) s, cy + (y - cy) s) for an affine g per (b, k); the f = 1 maps are the mirrored ones, stored in the
    partner channels.  -> stack (S*F*B, K, H, W) float32, g on the base grid (B, K, H, W) float64."""
    F = 2 if flip else 1
    cx, cy = W / 2.0, H / 2.0
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    bk = np.arange(B * K, dtype=np.float64).reshape(B, K, 1, 1)
    g = lambda xx, yy: (0.25 + 0.01 * bk) * xx - (0.125 + 0.02 * bk) * yy + 3.0 + bk
    stack = np.zeros((len(scales) * F * B, K, H, W), np.float32)
    for s, sc in enumerate(scales):
        m = g(cx + (x - cx) * sc, cy + (y - cy) * sc).astype(np.float32)
        stack[(s * F) * B:(s * F + 1) * B] = m
        if flip:
            stack[(s * F + 1) * B:(s * F + 2) * B][:, partner] = m[:, :, :, ::-1]
    return stack, g(x, y)
