"""Independent float64 numpy restatement of the movement spectrum (pk_motion_spectrum: DESIGN.md "Movement spectrum") and the case builders
its tests share.  The reference has no implementation, so this file pins the project's own specification:

  frequencies   exact rationals (j0 + j) / N; the phase of bin j at frame t is reduced in integers, r = ((j0 + j) t) mod N, and
                ang = 6.283185307179586 (r / N) lies in [0, 2 pi): the argument of sin / cos is bit-identical on the device and here.
  window        0 rectangular, 1 periodic Hann 0.5 - 0.5 cos(6.283185307179586 (t / T)); invalid frames weigh 0.
  power         P_j = (4 / (W W)) ((Xre^2 + Xim^2) + (Yre^2 + Yim^2)) of the weighted, mean-removed samples u_t = w_t (p_t - m).
  summary       n, W, band power, peak bin (lowest of equal maxima, -1 without power), peak power, centroid -- `summary` applies to any P.
"""
import functools

import numpy as np

import motion_np as mnp

F32, F64 = np.float32, np.float64
TWO_PI = 6.283185307179586
MAX_BINS, MAX_NFFT = 16384, 1 << 30


def window_weights(T, window):
    t = np.arange(T, dtype=F64)
    return np.ones(T) if window == 0 else 0.5 - 0.5 * np.cos(TWO_PI * (t / F64(T)))


def angles(T, N, j0, F):
    """(T, F) phase of bin j0 + j at frame t, reduced in int64 before it becomes a float."""
    r = (np.arange(j0, j0 + F, dtype=np.int64)[None, :] * np.arange(T, dtype=np.int64)[:, None]) % np.int64(N)
    return TWO_PI * (r.astype(F64) / F64(N))


def detrended(coords, conf=None, min_conf=0.3, window=1):
    """coords (S,T,K,2) -> n (S,K), W (S,K), u (S,T,K,2) float64 with zeros at invalid frames and for joints with n < 2 or W <= 0."""
    c = np.asarray(coords).astype(F64)                            # float32 widens exactly
    S, T, K, _ = c.shape
    ok = mnp.valid_frames(c, conf, min_conf)
    w = np.where(ok, window_weights(T, window)[None, :, None], 0.0)
    p = np.where(ok[..., None], c, 0.0)
    n, W = ok.sum(1), w.sum(1)
    live = (n >= 2) & (W > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (w[..., None] * p).sum(1) / W[..., None]
    u = np.where((ok & live[:, None, :])[..., None], w[..., None] * (p - m[:, None]), 0.0)
    return n, W, u, live


def power_scale(u, W, live):
    """The scale of a joint's power, 4 (sum_t |u_t.x| + |u_t.y|)^2 / W^2: no bin can exceed it, and the tolerance is relative to it."""
    a = np.abs(u).sum((1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(live, 4.0 * a * a / (W * W), 0.0)


def power(coords, conf, min_conf, N, j0, F, window):
    """-> P (S,K,F), n (S,K), W (S,K), scale (S,K)."""
    assert 2 <= N <= MAX_NFFT and j0 >= 1 and 1 <= F <= MAX_BINS and j0 + F - 1 <= N // 2 and window in (0, 1)
    n, W, u, live = detrended(coords, conf, min_conf, window)
    S, T, K, _ = u.shape
    ang = angles(T, N, j0, F)
    cs, sn = np.cos(ang), np.sin(ang)
    ut = np.moveaxis(u, 1, 2)                                     # (S,K,T,2)
    sq = np.zeros((S, K, F))
    for axis in (0, 1):
        re, im = ut[..., axis] @ cs, ut[..., axis] @ sn           # (S,K,F)
        sq += re * re + im * im
    with np.errstate(invalid="ignore", divide="ignore"):
        P = np.where(live[..., None], (4.0 / (W * W))[..., None] * sq, 0.0)
    return P, n.astype(F64), W, power_scale(u, W, live)


def summary(P, n, W, j0):
    """P (...,F), n and W (...) -> (...,6).  Sums in ascending j."""
    P = np.asarray(P, F64)
    out = np.zeros(P.shape[:-1] + (6,))
    out[..., 0], out[..., 1] = n, W
    band = np.zeros(P.shape[:-1])
    moment = np.zeros(P.shape[:-1])
    for j in range(P.shape[-1]):
        band = band + P[..., j]
        moment = moment + F64(j0 + j) * P[..., j]
    some = band != 0
    peak = P.argmax(-1)                                           # the first of equal maxima
    out[..., 2] = band
    out[..., 3] = np.where(some, j0 + peak, -1)
    out[..., 4] = np.where(some, np.take_along_axis(P, peak[..., None], -1)[..., 0], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., 5] = np.where(some, moment / band, 0.0)
    return out


def spectrum(coords, conf=None, min_conf=0.3, N=None, j0=1, F=None, window=1):
    """-> power (S,K,F), summary (S,K,6), scale (S,K)."""
    T = np.asarray(coords).shape[1]
    N = T if N is None else N
    F = N // 2 - j0 + 1 if F is None else F
    P, n, W, scale = power(coords, conf, min_conf, N, j0, F, window)
    return P, summary(P, n, W, j0), scale


# ------------------------------------------------------------------------------------------------ cases
def oscillation(T, N, m, amp=30.0, centre=(200.0, 300.0), direction=(0.6, 0.8), phase=0.4):
    """A linear oscillation of `amp` px along the unit vector `direction` at bin m of an N-point transform, float32."""
    t = np.arange(T)
    s = amp * np.cos(2 * np.pi * ((m * t) % N) / N + phase)
    return (np.asarray(centre)[None] + s[:, None] * np.asarray(direction)[None]).astype(F32)


def circle(T, N, m, radius=30.0, centre=(200.0, 300.0)):
    a = 2 * np.pi * ((m * np.arange(T)) % N) / N
    return (np.asarray(centre)[None] + radius * np.stack([np.cos(a), np.sin(a)], -1)).astype(F32)


@functools.lru_cache(maxsize=None)
def spectrum_case(S, T, K, with_conf, seed=0):
    """`motion_np.motion_case` (random walks; plain, never-valid, alternating, gappy and non-finite joints) with an oscillation of 12 px added
    to every joint at its own rate, and -- when there is room -- the LAST joint of the last sequence left with exactly one valid frame.
    Read-only arrays; conf is None without `with_conf`."""
    c0, conf0 = mnp.motion_case(S, T, K, with_conf, seed)
    c = c0.copy()
    conf = None if conf0 is None else conf0.copy()
    t = np.arange(T)
    for s in range(S):
        for k in range(K):
            c[s, :, k, 0] += (12.0 * np.sin(2 * np.pi * (0.03 + 0.02 * k + 0.01 * s) * t)).astype(F32)
    if S * K > 5 and T > 1:
        keep = T // 3
        for tt in range(T):
            if tt == keep:
                c[-1, tt, -1] = (100.0, 50.0)
                if conf is not None:
                    conf[-1, tt, -1] = 0.9
            elif conf is not None:
                conf[-1, tt, -1] = 0.1
            else:
                c[-1, tt, -1, 0] = np.nan
    c.setflags(write=False)
    if conf is not None:
        conf.setflags(write=False)
    return c, conf


def band_bins(fps, n_fft, f_min=None, f_max=None):
    """First bin and number of bins with f_min <= (j / n_fft) fps <= f_max among 1 .. n_fft // 2 (None: no limit on that side)."""
    j = np.arange(1, n_fft // 2 + 1)
    f = j / n_fft * fps
    sel = j[(f >= (-np.inf if f_min is None else f_min)) & (f <= (np.inf if f_max is None else f_max))]
    return (int(sel[0]), int(len(sel))) if len(sel) else (0, 0)
