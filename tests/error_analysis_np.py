"""Independent numpy restatements of the localisation error analysis (pk_kpt_error, pk_kpt_error_quantiles: DESIGN.md "Localisation error
analysis") and the case builders their tests share.

  errors           float32, operation by operation (numpy rounds every float32 operation once, as the kernel does without FMA); square root
                   and division in float64, then narrowed: equal to the correctly rounded float32 operations.
  calibration      the reference's loop over the bins (analysis/nn_quantitative_viz.py:171-178), one mask per bin.
  pr_reference     the reference's loop over the thresholds (:214-234): tp, fp, fn at every threshold.
  pr_hist          the histogram the kernel keeps instead: the number m of thresholds below each confidence.
  order_stats      np.sort.
  fixed_order_sum  the float64 sum in the kernel's order: per thread in ascending column, the xor butterfly inside each wave, then the
                   waves from left to right (`block_reduce` of pk_common.h).
Every output is an integer, an order statistic or that sum: the tests compare for equality.

The confidences are float32.  Edges and thresholds are rounded to float32 once (what the kernel reads) and compared in float32; the
reference compares with float64 linspace values, in float32 or float64 depending on the numpy version's promotion rule."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
THREADS, WAVE = 256, 64


# ------------------------------------------------------------------------------------------------ pk_kpt_error
def counted(pred, gt, vis, norm=None):
    ok = (np.asarray(vis, F32) > 0) & np.isfinite(np.asarray(pred, F32)).all(-1) & np.isfinite(np.asarray(gt, F32)).all(-1)
    if norm is not None:
        with np.errstate(invalid="ignore"):
            ok &= (np.asarray(norm, F32) > 0)[:, None]
    return ok


def errors(pred, gt, vis, norm=None):
    """-> (N,K) float32 errors, NaN for a pair that does not count (the store holds the transpose)."""
    pred, gt = np.asarray(pred, F32), np.asarray(gt, F32)
    ok = counted(pred, gt, vis, norm)
    with np.errstate(all="ignore"):
        dx, dy = pred[..., 0] - gt[..., 0], pred[..., 1] - gt[..., 1]
        d2 = dx * dx + dy * dy
        assert d2.dtype == F32
        e = np.sqrt(d2.astype(F64)).astype(F32)
        if norm is not None:
            e = (e.astype(F64) / np.asarray(norm, F32).astype(F64)[:, None]).astype(F32)
    return np.where(ok, e, F32(np.nan))


def calibration(err, conf, pixel_thr, edges):
    """err, conf (N,K) -> count, hit (K, n_bins) int64: the reference's loop, bin i takes edges[i] <= c < edges[i+1]."""
    err, conf, edges = np.asarray(err, F32), np.asarray(conf, F32), np.asarray(edges, F32)
    use = ~np.isnan(err) & np.isfinite(conf)
    accurate = err < F32(pixel_thr)
    K, nb = err.shape[1], len(edges) - 1
    count, hit = np.zeros((K, nb), np.int64), np.zeros((K, nb), np.int64)
    for k in range(K):
        c, a = conf[use[:, k], k], accurate[use[:, k], k]
        for i in range(nb):
            mask = (c >= edges[i]) & (c < edges[i + 1])
            count[k, i], hit[k, i] = mask.sum(), a[mask].sum()
    return count, hit


def pr_reference(err, conf, pixel_thr, thresholds):
    """err, conf (N,K) -> tp, fp, fn (K, T) int64: the reference's loop over the thresholds, per joint."""
    err, conf, thr = np.asarray(err, F32), np.asarray(conf, F32), np.asarray(thresholds, F32)
    use = ~np.isnan(err) & np.isfinite(conf)
    K, T = err.shape[1], len(thr)
    tp, fp, fn = (np.zeros((K, T), np.int64) for _ in range(3))
    for k in range(K):
        c, correct = conf[use[:, k], k], err[use[:, k], k] < F32(pixel_thr)
        for i in range(T):
            detected = c > thr[i]
            tp[k, i], fp[k, i], fn[k, i] = (detected & correct).sum(), (detected & ~correct).sum(), (~detected & correct).sum()
    return tp, fp, fn


def pr_hist(err, conf, pixel_thr, thresholds):
    """-> (K, 2, T+1) int64: [k, 0 correct / 1 not, m] counts the pairs with exactly m thresholds below their confidence."""
    err, conf, thr = np.asarray(err, F32), np.asarray(conf, F32), np.asarray(thresholds, F32)
    use = ~np.isnan(err) & np.isfinite(conf)
    K, T = err.shape[1], len(thr)
    out = np.zeros((K, 2, T + 1), np.int64)
    with np.errstate(invalid="ignore"):
        m = (conf[..., None] > thr).sum(-1)
        miss = (~(err < F32(pixel_thr))).astype(np.int64)
    n, k = np.nonzero(use)
    np.add.at(out, (k, miss[n, k], m[n, k]), 1)
    return out


def suffix_counts(hist):
    """tp, fp, fn (..., T) from pr_hist (..., 2, T+1), written as the sums of the specification."""
    hist = np.asarray(hist, np.int64)
    T = hist.shape[-1] - 1
    tp = np.stack([hist[..., 0, i + 1:].sum(-1) for i in range(T)], -1)
    fp = np.stack([hist[..., 1, i + 1:].sum(-1) for i in range(T)], -1)
    return tp, fp, hist[..., 0, :].sum(-1)[..., None] - tp


def reference_curves(tp, fp, fn):
    """precision, recall (T,) float64 and the reference's np.trapz(precisions, recalls) from the counts of its loop."""
    precision = np.array([t / (t + f) if t + f > 0 else 0 for t, f in zip(tp.tolist(), fp.tolist())], F64)
    recall = np.array([t / (t + f) if t + f > 0 else 0 for t, f in zip(tp.tolist(), fn.tolist())], F64)
    area = float((np.diff(recall) * (precision[1:] + precision[:-1]) / 2.0).sum())
    return precision, recall, area


REFERENCE_EDGES = np.linspace(0, 1, 11)                           # plot_confidence_vs_accuracy's bins
REFERENCE_THRESHOLDS = np.linspace(0, 1, 100)                     # plot_pr_curve's thresholds
PIXEL_THR = F32(10.0)


@functools.lru_cache(maxsize=None)
def error_case(N, K, with_norm, with_conf, seed=0):
    """Random predictions around random ground truth; some pairs invisible, NaN / inf coordinates, norm <= 0 and NaN confidences sprinkled
    in when there is room.  The first pairs of joint 0 are set by hand (as far as N reaches): pred == gt (error 0); an error exactly equal
    to the threshold (3-4-5 triangle scaled to 10: not a hit); confidences exactly on an inner bin edge, on the last edge, on a threshold
    and exactly 1.0.  -> pred, gt, vis, norm or None, conf or None, edges (float32), thresholds (float32).  Read-only arrays."""
    g = np.random.default_rng(7 * N + 131 * K + 2 * int(with_norm) + int(with_conf) + 1000 * seed)
    gt = (g.random((N, K, 2)) * [192, 256]).astype(F32)
    pred = (gt + g.standard_normal((N, K, 2)) * 8.0).astype(F32)
    vis = g.integers(0, 3, (N, K)).astype(F32)
    norm = (g.random(N) * 2 + 0.5).astype(F32) if with_norm else None
    conf = g.random((N, K)).astype(F32) if with_conf else None
    edges, thr = REFERENCE_EDGES.astype(F32), REFERENCE_THRESHOLDS.astype(F32)
    if N > 8:
        for v in (np.nan, np.inf, -np.inf):
            pred[g.integers(8, N), g.integers(0, K), g.integers(0, 2)] = v
            gt[g.integers(8, N), g.integers(0, K), g.integers(0, 2)] = v
        if with_norm:
            norm[g.integers(8, N, max(1, N // 50))] = 0.0
            norm[g.integers(8, N)] = -1.0
            norm[g.integers(8, N)] = np.nan
        if with_conf:
            conf[g.integers(8, N, max(1, N // 40)), g.integers(0, K, max(1, N // 40))] = np.nan
            conf[g.integers(8, N), g.integers(0, K)] = np.inf
            conf[g.integers(8, N), g.integers(0, K)] = -0.25     # below every edge and every threshold
            conf[g.integers(8, N), g.integers(0, K)] = 1.5       # above them
    hand = [((5, 7), (5, 7), edges[3]), ((6, 8), (0, 0), edges[-1]), ((1, 1), (2, 3), thr[37]), ((0, 0), (0, 3), F32(1.0)),
            ((50, 50), (50, 50.5), edges[0]), ((9, 9), (3, 1), thr[0])]
    for n, (p, q, c) in enumerate(hand[:N]):
        pred[n, 0], gt[n, 0], vis[n, 0] = p, q, 2
        if with_norm:
            norm[n] = 1.0
        if with_conf:
            conf[n, 0] = c
    for a in (pred, gt, vis, norm, conf, edges, thr):
        if a is not None:
            a.setflags(write=False)
    return pred, gt, vis, norm, conf, edges, thr


# ------------------------------------------------------------------------------------------------ pk_kpt_error_quantiles
def positions(n, q):
    """pos = q (double)(n - 1) -> lo = floor(pos), hi = min(lo + 1, n - 1), for n >= 1 and q in [0, 1]."""
    pos = F64(q) * F64(n - 1)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, n - 1)


def order_stats(row, q):
    """-> (Q,2) float32: v[lo], v[hi] of the non-NaN values of `row` in ascending order; zeros without one."""
    v = np.sort(np.asarray(row, F32)[~np.isnan(row)])
    out = np.zeros((len(q), 2), F32)
    for j, qj in enumerate(q):
        if len(v):
            lo, hi = positions(len(v), qj)
            out[j] = v[lo], v[hi]
    return out


def fixed_order_sum(row):
    """float64 sum of the non-NaN values in the kernel's order.  Thread t adds columns t, t + 256, ... in ascending order to 0.0 (a NaN
    column is skipped: the same as adding +0.0 to a non-negative sum); inside each wave of 64 threads the xor butterfly with offsets
    32, 16, ..., 1; then wave 0 + wave 1 + wave 2 + wave 3 from left to right."""
    v = np.asarray(row, F32).astype(F64)
    v = np.where(np.isnan(v), 0.0, v)
    v = np.concatenate([v, np.zeros(-len(v) % THREADS)]).reshape(-1, THREADS)
    with np.errstate(invalid="ignore"):
        s = np.zeros(THREADS)
        for chunk in v:
            s = s + chunk
        s = s.reshape(THREADS // WAVE, WAVE)
        lanes = np.arange(WAVE)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        t = s[0, 0]
        for w in range(1, THREADS // WAVE):
            t = t + s[w, 0]
    return t


def summary(row):
    """-> (4,) float64: n, sum, min, max of the non-NaN values; zeros without one."""
    v = np.asarray(row, F32)[~np.isnan(row)]
    if not len(v):
        return np.zeros(4)
    return np.array([len(v), fixed_order_sum(row), v.min(), v.max()], F64)


ROW_KINDS = ("empty", "single", "tied", "wide", "plain")


@functools.lru_cache(maxsize=None)
def store_case(n_cols, ld, seed=0):
    """A (5, ld) float32 store whose first n_cols columns hold: row 0 no value (all NaN); row 1 one value; row 2 heavily tied values (the
    distances of integer-grid points, every other one NaN when there is room); row 3 values spread log-uniformly over 1e-3 .. 1e4 plus 0,
    a subnormal and +inf (as far as n_cols reaches), so that every byte of the key discriminates; row 4 plain errors.  The columns from
    n_cols on hold a large finite number that must never be read as data.  Read-only."""
    g = np.random.default_rng(977 * n_cols + seed)
    s = np.full((5, ld), F32(3.0e38))
    s[:, :n_cols] = np.nan
    s[1, g.integers(0, n_cols)] = F32(2.5)
    dx, dy = g.integers(0, 4, n_cols), g.integers(0, 4, n_cols)
    s[2, :n_cols] = np.sqrt((dx * dx + dy * dy).astype(F64)).astype(F32)
    if n_cols > 8:
        s[2, 1:n_cols:2] = np.nan
    s[3, :n_cols] = (10.0 ** g.uniform(-3, 4, n_cols)).astype(F32)
    for i, v in enumerate((np.inf, 1e-42, 0.0)[:max(0, n_cols - 1)]):
        s[3, n_cols - 1 - i] = F32(v)
    s[4, :n_cols] = np.abs(g.standard_normal(n_cols) * 6.0).astype(F32)
    s.setflags(write=False)
    return s


QUANTILES = np.array([0.0, 1.0, 0.5, 0.25, 0.9, 0.05, 1.0 / 3.0], F64)
"""The ends, the median, and positions that are whole numbers for some rows (q = 0.5 of an odd count, q = 0.25 of 4 j + 1 values: the rows
of 257 values) and fractional for others."""
