"""numpy float64 restatement of the gradient-attribution units (csrc/pk_attribution.hip; rules: DESIGN.md "Gradient attribution"): the stem's
data gradient as the literal sum over taps and output channels, the unpacking of a packed gradient, the saliency reduction, Grad-CAM as
the kernel orders it (next to the reference's literal four lines, tests/test_attribution_host.py), and the seeding of the batched pass."""
import numpy as np

from occlusion_np import THREADS, WAVE, bf16_bits

F32, F64 = np.float32, np.float64


def bf16_round(a):
    """float -> the float64 value of its bf16 rounding (nearest even)."""
    return (bf16_bits(np.asarray(a, F32)).astype(np.uint32) << 16).view(F32).astype(F64)


def from_bits(u16):
    return (np.asarray(u16, np.uint16).astype(np.uint32) << 16).view(F32)


# ------------------------------------------------------------------------------------------------ stem data gradient
def stem_dgrad(g, w, Hs, Ws, c_real=3):
    """g (B,Ho,Wo,Cout), w the forward pack (Cout,9,8) -> (dx, mag), both (B,Hs,Ws,8) float64: dx[b,y,x,c] = sum over the taps (ky,kx) with
    y + 1 - ky and x + 1 - kx even and inside the output, and over n, of g[b,oy,ox,n] w[n,ky 3 + kx,c]; mag is the same sum over the
    absolute values of the terms (the scale of its rounding error).  Channels >= c_real are 0."""
    g, w = np.asarray(g, F64), np.asarray(w, F64)
    B, Ho, Wo, Cout = g.shape
    assert w.shape == (Cout, 9, 8) and Ho == (Hs - 1) // 2 + 1 and Wo == (Ws - 1) // 2 + 1
    dx, mag = np.zeros((B, Hs, Ws, 8)), np.zeros((B, Hs, Ws, 8))
    for y in range(Hs):
        for x in range(Ws):
            for ky in range(3):
                for kx in range(3):
                    ty, tx = y + 1 - ky, x + 1 - kx
                    if ty % 2 or tx % 2 or not (0 <= ty // 2 < Ho and 0 <= tx // 2 < Wo):
                        continue
                    row = g[:, ty // 2, tx // 2, :]                       # (B, Cout)
                    dx[:, y, x, :c_real] += row @ w[:, ky * 3 + kx, :c_real]
                    mag[:, y, x, :c_real] += np.abs(row) @ np.abs(w[:, ky * 3 + kx, :c_real])
    return dx, mag


def pack_weight(w_oihw):
    """(Cout,Cin,3,3) -> the forward pack (Cout,9,8): [n][ky 3 + kx][c], channels >= Cin zero."""
    w = np.asarray(w_oihw, F64)
    Cout, Cin = w.shape[:2]
    out = np.zeros((Cout, 9, 8))
    out[:, :, :Cin] = w.reshape(Cout, Cin, 9).transpose(0, 2, 1)
    return out


# ------------------------------------------------------------------------------------------------ packed gradient
def nhwc_to_nchw(bits, C):
    """(B,H,W,Cpad) uint16 bf16 bits -> (B,C,H,W) float32, exact."""
    return np.ascontiguousarray(np.moveaxis(from_bits(bits)[..., :C], -1, 1))


def saliency(bits, c_real=3):
    """(B,H,W,8) uint16 bf16 bits -> (B,H,W) float32: max over c < c_real of |g_c|, a NaN in a real channel giving NaN (np.max's rule)."""
    with np.errstate(invalid="ignore"):
        return np.max(np.abs(from_bits(bits)[..., :c_real]), axis=-1)


# ------------------------------------------------------------------------------------------------ Grad-CAM
def _block_sum(cols):
    """(n, C) float64 -> (C,): per column the kernel's sum: thread t adds rows t, t + 256, ... in ascending order to 0.0, the xor butterfly
    32 .. 1 inside each wave, then wave 0 + 1 + 2 + 3."""
    n, C = cols.shape
    pad = -n % THREADS
    v = np.concatenate([cols, np.zeros((pad, C))]).reshape(-1, THREADS, C)       # + 0.0 changes nothing a sum started at 0.0 can hold
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((THREADS, C))
        for chunk in v:
            s = s + chunk
        s = s.reshape(THREADS // WAVE, WAVE, C)
        lanes = np.arange(WAVE)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        t = s[0, 0]
        for wv in range(1, THREADS // WAVE):
            t = t + s[wv, 0]
    return t


def grad_cam(A, G, c_used=None):
    """A, G (B,h,w,C) -> cam (B,h,w) float32, weights (B,c_used) float32, range (B,2) float64, in the kernel's order: weights = block sum
    / (h w); raw = max(0, sum over c ascending of weights[c] A[..., c]) with a NaN staying; cam = (raw - min) / ((max - min) + 1e-8);
    a NaN in any raw value makes the sample's range and map NaN."""
    A, G = np.asarray(A, F64), np.asarray(G, F64)
    B, h, w, C = A.shape
    c_used = C if c_used is None else c_used
    cam, wts, rng = np.zeros((B, h, w), F32), np.zeros((B, c_used), F32), np.zeros((B, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            wt = _block_sum(G[b].reshape(h * w, C)[:, :c_used]) / F64(h * w)
            a = A[b].reshape(h * w, C)
            s = np.zeros(h * w)
            for c in range(c_used):
                s = s + wt[c] * a[:, c]
            raw = np.where((s > 0) | np.isnan(s), s, 0.0)
            lo, hi = (np.nan, np.nan) if np.isnan(raw).any() else (raw.min(), raw.max())
            cam[b] = ((raw - lo) / ((hi - lo) + 1e-8)).reshape(h, w).astype(F32)
            wts[b], rng[b] = wt.astype(F32), (lo, hi)
    return cam, wts, rng


def grad_cam_literal(A, G):
    """The reference's four lines (analysis/nn_quantitative_viz.py:404-413) on ONE sample in the reference's (1,C,h,w) layout, float64."""
    weights = G.mean(axis=(2, 3), keepdims=True)
    cam = (weights * A).sum(axis=1, keepdims=True)
    cam = np.maximum(cam, 0.0)
    cam = cam - cam.min()
    return cam / (cam.max() + 1e-8)


# ------------------------------------------------------------------------------------------------ the batched seeding
def seed(joints, K, h, w):
    """d score / d heatmaps of the batched pass, score = sum_i heatmaps[i, joints[i]].sum(): copy i has ones over map joints[i]."""
    s = np.zeros((len(joints), K, h, w), F32)
    for i, j in enumerate(joints):
        s[i, j] = 1.0
    return s
