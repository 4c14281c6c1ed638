"""Independent float64 numpy restatement of the limb kinematics (csrc/pk_kinematics.hip: DESIGN.md "Limb kinematics") and the case builders
its tests share.  The reference has no implementation, so this file pins the project's own specification:

  angles    theta = arctan2(|u.x v.y - u.y v.x|, u.x v.x + u.y v.y), u = p_a - p_b, v = p_c - p_b, NaN for an invalid joint or a ray of length 0
  speeds    sqrt(dx dx + dy dy) of p[t+1] - p[t] when both frames are valid, else NaN
  series    float64 (S,T,Q), an element is valid iff finite
  stats     n, min, max, mean, population sd about that mean, sum |step|, steps, largest step
  xcorr     per lag Pearson's r of the co-valid pairs about THEIR means, 0 when n < 2 or not sxx syy > 0; summary over the lags with enough pairs
  entropy   |W|, B, A: valid templates and the pairs i < j within tol over m and m + 1 elements; fabs(a - b) <= tol, equality matches

Sums are taken in one of two orders: "ascending" (one running sum) or "tree", the device's: thread i of 256 adds elements i, i + 256, ...
in ascending order, then the xor butterfly of each 64-lane wave (offsets 32 .. 1), then the four waves from left to right.  A skipped
(invalid) element and an added +0.0 give the same bits, so invalid terms are zeros here."""
import numpy as np

import motion_np as mnp

F32, F64 = np.float32, np.float64
MAX_ANGLES, MAX_LAG, MAX_M, MAX_T, STATS_COLS = 64, 4096, 4, 262144, 8
COCO_ANGLES = {"left_elbow": (5, 7, 9), "right_elbow": (6, 8, 10), "left_shoulder": (7, 5, 11), "right_shoulder": (8, 6, 12),
               "left_hip": (5, 11, 13), "right_hip": (6, 12, 14), "left_knee": (11, 13, 15), "right_knee": (12, 14, 16)}


# ------------------------------------------------------------------------------------------------ angles and speeds
def joint_angles(coords, conf, min_conf, triples):
    """coords (S,T,K,2) float32, conf (S,T,K) or None, triples [(a, b, c)] -> (S,T,A) float64 radians."""
    c = np.asarray(coords).astype(F64)                            # float32 widens exactly
    ok = mnp.valid_frames(c, conf, min_conf)
    out = np.full(c.shape[:2] + (len(triples),), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, (a, b, cc) in enumerate(triples):
            u, v = c[:, :, a] - c[:, :, b], c[:, :, cc] - c[:, :, b]
            cr = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
            dt = u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]
            live = ok[:, :, a] & ok[:, :, b] & ok[:, :, cc] & (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1] > 0) \
                & (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] > 0)
            out[:, :, j] = np.where(live, np.arctan2(np.abs(cr), dt), np.nan)
    return out


def joint_speeds(coords, conf=None, min_conf=0.3):
    """-> (S,T,K) float64; the last frame is NaN."""
    c = np.asarray(coords).astype(F64)
    ok = mnp.valid_frames(c, conf, min_conf)
    out = np.full(c.shape[:3], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        d = c[:, 1:] - c[:, :-1]
        out[:, :-1] = np.where(ok[:, 1:] & ok[:, :-1], np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]), np.nan)
    return out


# ------------------------------------------------------------------------------------------------ ordered sums
def tree_sum(v):
    """Sum over the LAST axis in the device's order."""
    v = np.asarray(v, F64)
    n = v.shape[-1]
    chunks = max(1, -(-n // 256))
    pad = np.zeros(v.shape[:-1] + (chunks * 256,))
    pad[..., :n] = v
    part = pad.reshape(v.shape[:-1] + (chunks, 256))
    acc = np.zeros(v.shape[:-1] + (256,))
    for c in range(chunks):
        acc = acc + part[..., c, :]
    acc = acc.reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    red = acc[..., 0]
    return ((red[..., 0] + red[..., 1]) + red[..., 2]) + red[..., 3]


def ascending_sum(v):
    v = np.asarray(v, F64)
    return np.cumsum(v, axis=-1)[..., -1] if v.shape[-1] else np.zeros(v.shape[:-1])


def _sum(order):
    return {"ascending": ascending_sum, "tree": tree_sum}[order]


# ------------------------------------------------------------------------------------------------ statistics of a series
def series_stats(series, mean=None, order="ascending"):
    """series (S,T,Q) -> (S,Q,8).  `mean` (S,Q): use these bits as the mean of column 4 and store them in column 3 (the device's own)."""
    x = np.moveaxis(np.asarray(series, F64), 1, 2)                # (S,Q,T)
    osum = _sum(order)
    ok = np.isfinite(x)
    z = np.where(ok, x, 0.0)
    n = ok.sum(-1)
    out = np.zeros(x.shape[:2] + (STATS_COLS,))
    some = n > 0
    out[..., 0] = n
    out[..., 1] = np.where(some, np.where(ok, x, np.inf).min(-1, initial=np.inf), 0.0)
    out[..., 2] = np.where(some, np.where(ok, x, -np.inf).max(-1, initial=-np.inf), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(some, osum(z) / n, 0.0) if mean is None else np.asarray(mean, F64)
        d = np.where(ok, x - m[..., None], 0.0)
        out[..., 3] = m
        out[..., 4] = np.where(some, np.sqrt(osum(d * d) / n), 0.0)
    step_ok = ok[..., 1:] & ok[..., :-1]
    with np.errstate(invalid="ignore"):
        step = np.where(step_ok, np.abs(x[..., 1:] - x[..., :-1]), 0.0)
    out[..., 5], out[..., 6], out[..., 7] = osum(step), step_ok.sum(-1), step.max(-1, initial=0.0)
    return out


# ------------------------------------------------------------------------------------------------ cross-correlation
def lag_pairs(xi, xj, lag):
    """(..., T) series -> x, y (..., T - |lag|) of one lag, in the order of the earlier frame of each pair; empty for |lag| >= T."""
    T = xi.shape[-1]
    span = max(T - abs(lag), 0)
    if lag >= 0:
        return xi[..., :span], xj[..., lag:lag + span]
    return xi[..., -lag:-lag + span], xj[..., :span]


def xcorr(series, pairs, max_lag, order="ascending"):
    """series (S,T,Q), pairs [(i, j)] -> corr (S,P,2L+1) float64, count (S,P,2L+1) int32."""
    s = np.asarray(series, F64)
    S, T, Q = s.shape
    L, osum = int(max_lag), _sum(order)
    corr = np.zeros((S, len(pairs), 2 * L + 1))
    count = np.zeros((S, len(pairs), 2 * L + 1), np.int32)
    for p, (i, j) in enumerate(pairs):
        for li in range(2 * L + 1):
            x, y = lag_pairs(s[:, :, i], s[:, :, j], li - L)
            if x.shape[-1] == 0:
                continue
            ok = np.isfinite(x) & np.isfinite(y)
            n = ok.sum(-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                mx, my = osum(np.where(ok, x, 0.0)) / n, osum(np.where(ok, y, 0.0)) / n
                dx, dy = np.where(ok, x - mx[:, None], 0.0), np.where(ok, y - my[:, None], 0.0)
                sxx, syy, sxy = osum(dx * dx), osum(dy * dy), osum(dx * dy)
                den = sxx * syy
                corr[:, p, li] = np.where((n >= 2) & (den > 0), sxy / np.sqrt(den), 0.0)
            count[:, p, li] = n
    return corr, count


def xcorr_summary(corr, count, min_count=2):
    """corr, count (..., 2L+1) -> (..., 4): r at lag 0, the lag of the largest r (the lowest among equal maxima), that r, its count."""
    corr, count = np.asarray(corr, F64), np.asarray(count)
    L = (corr.shape[-1] - 1) // 2
    ok = count >= min_count
    out = np.zeros(corr.shape[:-1] + (4,))
    out[..., 0] = np.where(ok[..., L], corr[..., L], 0.0)
    best = np.where(ok, corr, -np.inf).argmax(-1)                 # the first of equal maxima
    some = ok.any(-1)
    out[..., 1] = np.where(some, best - L, 0)
    out[..., 2] = np.where(some, np.take_along_axis(corr, best[..., None], -1)[..., 0], 0.0)
    out[..., 3] = np.where(some, np.take_along_axis(count, best[..., None], -1)[..., 0], 0)
    return out


# ------------------------------------------------------------------------------------------------ sample entropy
def template_starts(x, m):
    """Valid template starts W of one series (T,): i <= T - m - 1 with x[i .. i + m] all finite."""
    T = len(x)
    if T - m <= 0:
        return np.zeros(0, np.int64)
    fin = np.isfinite(x)
    ok = np.ones(T - m, bool)
    for k in range(m + 1):
        ok &= fin[k:k + T - m]
    return np.flatnonzero(ok)


def entropy_counts_1d(x, tol, m):
    """-> (|W|, B, A) of one series (T,) by the all-pairs definition."""
    x = np.asarray(x, F64)
    w = template_starts(x, m)
    if not (np.isfinite(tol) and tol >= 0) or len(w) < 2:
        return len(w), 0, 0
    match = np.triu(np.ones((len(w), len(w)), bool), 1)           # i < j
    for k in range(m):
        e = x[w + k]
        match &= np.abs(e[:, None] - e[None, :]) <= tol
    e = x[w + m]
    return len(w), int(match.sum()), int((match & (np.abs(e[:, None] - e[None, :]) <= tol)).sum())


def sample_entropy_counts(series, tol, m=2):
    """series (S,T,Q), tol (S,Q) -> (S,Q,3) int64."""
    s, tol = np.asarray(series, F64), np.asarray(tol, F64)
    S, T, Q = s.shape
    out = np.zeros((S, Q, 3), np.int64)
    for a in range(S):
        for q in range(Q):
            out[a, q] = entropy_counts_1d(s[a, :, q], tol[a, q], m)
    return out


def sample_entropy(counts):
    """(|W|, B, A) -> -ln(A / B), or None when A or B is 0."""
    _, B, A = (int(v) for v in counts)
    return None if A == 0 or B == 0 else float(-np.log(A / B))


def entropy_tiles(T, m, tile=256):
    nb = 0 if T - m <= 0 else -(-(T - m) // tile)
    return nb * (nb + 1) // 2 if 0 < T <= MAX_T and 1 <= m <= MAX_M else 0


# ------------------------------------------------------------------------------------------------ cases
def kinematics_case(S, T, K, seed=0):
    """Seeded random walks in a 640 x 480 frame with NaN / +-inf coordinates sprinkled in and confidences on both sides of 0.3 (one exactly
    at it).  -> coords (S,T,K,2) float32, conf (S,T,K) float32, writable copies."""
    g = np.random.default_rng(1009 * S + 17 * T + K + seed)
    c = (np.array([320.0, 240.0]) + 40.0 * g.standard_normal((S, 1, K, 2)) + np.cumsum(g.standard_normal((S, T, K, 2)) * 3.0, axis=1)).astype(F32)
    conf = (0.3 + 0.7 * g.random((S, T, K))).astype(F32)
    n = max(1, S * T * K // 16)
    for v in (np.nan, np.inf, -np.inf):
        c[g.integers(0, S, n // 4 + 1), g.integers(0, T, n // 4 + 1), g.integers(0, K, n // 4 + 1), g.integers(0, 2, n // 4 + 1)] = v
    conf[g.integers(0, S, n), g.integers(0, T, n), g.integers(0, K, n)] = (0.29 * g.random(n)).astype(F32)
    conf[0, T // 2, 0] = F32(0.3)                                 # exactly at the threshold counts
    conf[g.integers(0, S), g.integers(0, T), g.integers(0, K)] = np.nan
    return c, conf


def series_case(S, T, Q, seed=0, gap_share=0.1):
    """Seeded float64 series (S,T,Q): smooth drift plus noise, NaN gaps in about `gap_share` of the elements, series 1 (if any) all NaN and
    series 2 (if any) with a single valid element."""
    g = np.random.default_rng(7 * S + 131 * T + Q + seed)
    x = np.cumsum(g.standard_normal((S, T, Q)), axis=1) * 0.3 + g.standard_normal((S, T, Q))
    x[g.random((S, T, Q)) < gap_share] = np.nan
    if Q > 1:
        x[:, :, 1] = np.nan
    if Q > 2:
        x[:, :, 2] = np.nan
        x[:, T // 2, 2] = 1.25
    return x


def elbow_trajectory(T=300, lag=6, lo_deg=40.0, hi_deg=150.0, period=48.0, seed=3):
    """A 17-joint (T,17,2) float32 trajectory: shoulders and elbows fixed, each wrist on a circle of 50 px about its elbow so that the elbow
    angle runs sinusoidally between lo_deg and hi_deg; the RIGHT elbow repeats the left one `lag` frames later.  The left knee's ankle is
    driven by seeded noise; every other joint rests."""
    g = np.random.default_rng(seed)
    seq = np.zeros((T, 17, 2), F64)
    seq[:] = np.stack([100.0 + 20.0 * np.arange(17), 200.0 + 7.0 * np.arange(17)], -1)[None]

    def angle(t):
        return np.deg2rad(0.5 * (lo_deg + hi_deg) + 0.5 * (hi_deg - lo_deg) * np.sin(2 * np.pi * t / period))

    t = np.arange(T, dtype=F64)
    for sh, el, wr, shift, x0 in ((5, 7, 9, 0, 200.0), (6, 8, 10, lag, 400.0)):
        seq[:, sh], seq[:, el] = (x0, 100.0), (x0, 180.0)        # the upper arm points straight up from the elbow
        th = angle(t - shift)
        seq[:, wr, 0], seq[:, wr, 1] = x0 + 50.0 * np.sin(th), 180.0 - 50.0 * np.cos(th)
    seq[:, 11], seq[:, 13] = (250.0, 300.0), (250.0, 380.0)
    th = np.deg2rad(g.uniform(30.0, 150.0, T))
    seq[:, 15, 0], seq[:, 15, 1] = 250.0 + 50.0 * np.sin(th), 380.0 - 50.0 * np.cos(th)
    return seq.astype(F32)
