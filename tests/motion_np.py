"""Independent numpy restatements of the movement-analysis and PCK kernels (pk_pck, pk_motion_stats, pk_position_histogram: DESIGN.md
"Movement analysis and PCK") and the case builders their tests share.  The reference has no implementation of these functions, so this
file pins the project's own specification:

  pck            float32, operation by operation (numpy rounds every float32 operation once, as the kernel does without FMA): the counts are
                 integers and must be EQUAL; err_sum is float64.
  motion_stats   float64 on the exactly widened float32 inputs.
  bin_index      the guess-and-walk bin rule; `position_histogram` applies it, the tests compare both with np.histogram2d.
"""
import functools

import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ PCK
def pck(pred, gt, vis, norm, thresholds):
    """-> correct (n_thr,K) int64, valid (K,) int64, err_sum (K,) float64."""
    pred, gt, vis = np.asarray(pred, F32), np.asarray(gt, F32), np.asarray(vis, F32)
    norm, thr = np.asarray(norm, F32), np.asarray(thresholds, F32)
    ok = (vis > 0) & (norm[:, None] > 0) & np.isfinite(pred).all(-1) & np.isfinite(gt).all(-1)
    with np.errstate(all="ignore"):
        dx, dy = pred[..., 0] - gt[..., 0], pred[..., 1] - gt[..., 1]
        d2 = dx * dx + dy * dy                                   # float32: two products, one sum, each rounded once
        r = thr[:, None, None] * norm[None, :, None]
        hit = (d2[None] <= r * r) & ok[None]
        err = np.where(ok, np.sqrt(d2.astype(F64)) / norm.astype(F64)[:, None], 0.0)
    assert d2.dtype == F32 and r.dtype == F32
    return hit.sum(1).astype(np.int64), ok.sum(0).astype(np.int64), err.sum(0)


TIE_NORM, TIE_THR = F32(8.0), F32(0.5)                            # r = 4, r r = 16
TIE_DY = F32(2.0 ** -9.5)                                        # dy dy rounds to 2^-19 (1 +- 2^-24) = one float32 ulp of 16


@functools.lru_cache(maxsize=None)
def pck_case(N, K, n_thr, seed=0):
    """Random predictions around random ground truth, normalisers of box size; some pairs invisible, some samples with norm 0, some
    coordinates NaN / inf.  Threshold 0 is TIE_THR; joint 0 of sample 0 sits exactly ON the circle of TIE_THR (d2 == r r: a hit) and,
    when N > 1, joint 0 of sample 1 one float32 ulp of d2 outside it (a miss).  Read-only arrays."""
    g = np.random.default_rng(1000 * N + 10 * K + n_thr + seed)
    gt = (g.random((N, K, 2)) * [192, 256]).astype(F32)
    norm = (g.random(N) * 200 + 20).astype(F32)
    pred = (gt + g.standard_normal((N, K, 2)) * norm[:, None, None] * 0.25).astype(F32)
    vis = g.integers(0, 3, (N, K)).astype(F32)
    thr = np.concatenate([[TIE_THR], np.linspace(0.05, 1.0, n_thr - 1)]).astype(F32) if n_thr > 1 else np.array([TIE_THR], F32)
    if N > 8:
        norm[g.integers(2, N, max(1, N // 50))] = 0.0
        norm[g.integers(2, N)] = -1.0
        for v in (np.nan, np.inf, -np.inf):
            pred[g.integers(2, N), g.integers(0, K), g.integers(0, 2)] = v
            gt[g.integers(2, N), g.integers(0, K), g.integers(0, 2)] = v
    gt[0, 0], pred[0, 0], vis[0, 0], norm[0] = (0, 0), (4, 0), 2, TIE_NORM
    if N > 1:
        gt[1, 0], pred[1, 0], vis[1, 0], norm[1] = (0, 0), (4, TIE_DY), 1, TIE_NORM
    for a in (pred, gt, vis, norm, thr):
        a.setflags(write=False)
    return pred, gt, vis, norm, thr


# ------------------------------------------------------------------------------------------------ movement statistics
def valid_frames(coords, conf=None, min_conf=0.3):
    ok = np.isfinite(np.asarray(coords)).all(-1)
    if conf is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(conf, F32) >= F32(min_conf)
    return ok


def motion_stats(coords, conf=None, min_conf=0.3):
    """coords (S,T,K,2) float32 or float64, conf (S,T,K) or None -> (S,K,11) float64."""
    c = np.asarray(coords).astype(F64)                            # float32 (what the kernel reads) widens exactly; float64 stays
    S, T, K, _ = c.shape
    ok = valid_frames(c, conf, min_conf)
    p = np.where(ok[..., None], c, 0.0)                           # invalid frames never enter a counted term
    out = np.zeros((S, K, 11))
    out[..., 0] = ok.sum(1)
    some = out[..., 0] > 0
    for col, axis, fn, fill in ((1, 0, np.min, np.inf), (2, 0, np.max, -np.inf), (3, 1, np.min, np.inf), (4, 1, np.max, -np.inf)):
        out[..., col] = np.where(some, fn(np.where(ok, p[..., axis], fill), axis=1), 0.0)
    rx, ry = out[..., 2] - out[..., 1], out[..., 4] - out[..., 3]
    out[..., 5] = np.sqrt(rx * rx + ry * ry)
    step_ok = ok[:, 1:] & ok[:, :-1]
    d = p[:, 1:] - p[:, :-1]
    step = np.where(step_ok, np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]), 0.0)
    out[..., 6], out[..., 7], out[..., 8] = step.sum(1), step_ok.sum(1), step.max(1, initial=0.0)
    tri_ok = ok[:, 2:] & ok[:, 1:-1] & ok[:, :-2]
    a = (p[:, 2:] - 2.0 * p[:, 1:-1]) + p[:, :-2]
    acc = np.where(tri_ok, np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]), 0.0)
    out[..., 9], out[..., 10] = acc.sum(1), tri_ok.sum(1)
    return out


KINDS = ("plain", "never valid", "alternating", "gap", "non-finite")


def joint_kind(s, k, K, seed):
    return KINDS[(s * K + k + seed) % len(KINDS)]


@functools.lru_cache(maxsize=None)
def motion_case(S, T, K, with_conf, seed=0):
    """Random walks in a 640 x 480 frame.  Joint (s,k) is of kind `joint_kind(s, k, K, seed)`: plain; never valid; valid in alternating
    frames only (no step anywhere); one invalid frame in the middle (it breaks the two steps that touch it and the three triples that
    hold it); NaN / +inf / -inf coordinates sprinkled in.  Invalid means a confidence below the threshold with `with_conf` (a plain joint
    then also has one confidence exactly AT the threshold, which counts), NaN coordinates without.  Read-only arrays; conf is None
    without `with_conf`."""
    g = np.random.default_rng(7919 * S + 31 * T + K + 2 * seed + int(with_conf))
    c = (np.array([320.0, 240.0]) + np.cumsum(g.standard_normal((S, T, K, 2)) * 3.0, axis=1)).astype(F32)
    conf = (0.5 + 0.5 * g.random((S, T, K))).astype(F32) if with_conf else None

    def drop(s, t, k):
        if with_conf:
            conf[s, t, k] = g.random() * 0.29
        else:
            c[s, t, k, g.integers(0, 2)] = np.nan

    for s in range(S):
        for k in range(K):
            kind = joint_kind(s, k, K, seed)
            if kind == "never valid":
                for t in range(T):
                    drop(s, t, k)
            elif kind == "alternating":
                for t in range(1, T, 2):
                    drop(s, t, k)
            elif kind == "gap":
                drop(s, T // 2, k)
            elif kind == "non-finite":
                for v in (np.nan, np.inf, -np.inf):
                    c[s, g.integers(0, T), k, g.integers(0, 2)] = v
            elif with_conf:
                conf[s, g.integers(0, T), k] = F32(0.3)
    c.setflags(write=False)
    if conf is not None:
        conf.setflags(write=False)
    return c, conf


# ------------------------------------------------------------------------------------------------ position histogram
def bin_index(v, edges):
    """Bin of one value for ascending float64 `edges`: e[i] <= v < e[i+1], the last bin right-inclusive, -1 outside [e[0], e[-1]] and
    for NaN.  A float64 guess from the end edges, clamped, then a walk along the edges."""
    e, nb, v = np.asarray(edges, F64), len(edges) - 1, float(v)
    if not (e[0] <= v <= e[nb]):
        return -1
    i = int(min(max(np.floor((v - e[0]) / (e[nb] - e[0]) * nb), 0), nb - 1))
    while i > 0 and v < e[i]:
        i -= 1
    while i < nb - 1 and v >= e[i + 1]:
        i += 1
    return i


def position_histogram(coords, edges_x, edges_y, conf=None, min_conf=0.3):
    """coords (S,T,K,2) -> (S,K,nby,nbx) int32 by `bin_index`."""
    c = np.asarray(coords, F32)
    S, T, K, _ = c.shape
    ok = valid_frames(c, conf, min_conf)
    out = np.zeros((S, K, len(edges_y) - 1, len(edges_x) - 1), np.int32)
    for s, t, k in zip(*np.nonzero(ok)):
        bx, by = bin_index(c[s, t, k, 0], edges_x), bin_index(c[s, t, k, 1], edges_y)
        if bx >= 0 and by >= 0:
            out[s, k, by, bx] += 1
    return out


def histogram2d(coords, edges_x, edges_y, conf=None, min_conf=0.3):
    """The same counts from np.histogram2d, joint by joint (rows = y)."""
    c = np.asarray(coords, F32)
    S, T, K, _ = c.shape
    ok = valid_frames(c, conf, min_conf)
    out = np.zeros((S, K, len(edges_y) - 1, len(edges_x) - 1), np.int32)
    for s in range(S):
        for k in range(K):
            x, y = c[s, ok[s, :, k], k, 0].astype(F64), c[s, ok[s, :, k], k, 1].astype(F64)
            out[s, k] = np.histogram2d(x, y, bins=[np.asarray(edges_x, F64), np.asarray(edges_y, F64)])[0].T
    return out


def edge_points(W, H, nbx, nby):
    """float32 (x, y) points that try the bin rule: every edge (rounded to float32) and its float32 neighbours, 0, -0.0, W, H, one ulp
    either side of W and H, points outside the range, NaN and infinities."""
    ex, ey = np.linspace(0, W, nbx + 1), np.linspace(0, H, nby + 1)

    def axis(e, top):
        v = [F32(x) for x in e]
        v += [np.nextafter(F32(x), F32(np.inf)) for x in e] + [np.nextafter(F32(x), F32(-np.inf)) for x in e]
        v += [F32(0.0), F32(-0.0), F32(top), np.nextafter(F32(top), F32(np.inf)), np.nextafter(F32(top), F32(0)), F32(-1.0), F32(top + 5.0),
              F32(np.nan), F32(np.inf), F32(-np.inf), F32(top / 3.0)]
        return np.array(v, F32)

    xs, ys = axis(ex, W), axis(ey, H)
    n = max(len(xs), len(ys))
    xs, ys = np.resize(xs, n), np.resize(ys, n)
    # every x special against an interior y, every y special against an interior x, and the specials against each other
    pts = np.concatenate([np.stack([xs, np.full(n, F32(H / 2.0 + 0.25))], -1), np.stack([np.full(n, F32(W / 2.0 + 0.25)), ys], -1),
                          np.stack([xs, ys], -1), np.stack([xs, ys[::-1]], -1)])
    return pts.astype(F32)


@functools.lru_cache(maxsize=None)
def histogram_case(S, T, K, W, H, nbx, nby, with_conf, seed=0):
    """T frames per joint: the `edge_points` (as many as fit, a different stretch of them per joint) followed by random positions in and
    slightly around the image.  -> coords (S,T,K,2), conf (S,T,K) or None, edges_x, edges_y.  Read-only arrays."""
    g = np.random.default_rng(104729 + 17 * T + S * K + nbx + seed + int(with_conf))
    c = (g.random((S, T, K, 2)) * [W * 1.1, H * 1.1] - [W * 0.05, H * 0.05]).astype(F32)
    pts = edge_points(W, H, nbx, nby)
    for s in range(S):
        for k in range(K):
            take = np.roll(pts, -(s * K + k) * max(1, T // 2), axis=0)[:T]
            c[s, :len(take), k] = take
    conf = g.random((S, T, K)).astype(F32) if with_conf else None
    ex, ey = np.linspace(0, W, nbx + 1), np.linspace(0, H, nby + 1)
    for a in (c, conf, ex, ey):
        if a is not None:
            a.setflags(write=False)
    return c, conf, ex, ey


# ------------------------------------------------------------------------------------------------ report
def quick_start_wrists(T=300):
    """The two wrists of the reference's clinical example (examples/quick_start.py:221-232): 10 s, amplitude 30 px, frequency 0.5 Hz, the
    right wrist a phase pi/4 ahead.  -> (T, 2, 2) float32: joint 0 = left, joint 1 = right."""
    t = np.linspace(0, 10, T)
    amp, freq = 30.0, 0.5
    left = np.stack([200 + amp * np.sin(2 * np.pi * freq * t), 300 + amp * np.cos(2 * np.pi * freq * t)], -1)
    right = np.stack([400 + amp * np.sin(2 * np.pi * freq * t + np.pi / 4), 300 + amp * np.cos(2 * np.pi * freq * t + np.pi / 4)], -1)
    return np.stack([left, right], 1).astype(F32)


def asymmetry_ratio(a_left, a_right):
    return abs(a_left - a_right) / max(a_left, a_right) if max(a_left, a_right) > 0 else 0.0


def flag(amplitude, min_movement=5.0, max_movement=200.0):
    return "low" if amplitude < min_movement else ("high" if amplitude > max_movement else None)
