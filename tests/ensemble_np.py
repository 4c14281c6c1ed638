"""numpy float64 restatement of the ensemble unit (csrc/pk_ensemble.hip), written from the text in include/posekernels.h (rules: DESIGN.md
"Predictive uncertainty"): the per-element moments with explicit ascending loops over the members, and the per-point rows in the
thread-stride plus butterfly order of `block_reduce`, as tests/occlusion_np.py restates pk_heatmap_summary."""
import numpy as np

F32, F64 = np.float32, np.float64
THREADS, WAVE = 256, 64
COLS = 12


# ------------------------------------------------------------------------------------------------ moments
def moments(stack, ddof=0):
    """(S, ...) float32 -> mean, std (...) float32.  Per element in float64: m = (((0 + v_0) + v_1) + ...) / S, q = the sum of (v_s - m)^2
    in ascending s, std = sqrt(q / (S - ddof)); both narrowed to float32 (numpy rounds to nearest even)."""
    v = np.asarray(stack, F32)
    S = v.shape[0]
    assert ddof in (0, 1) and S >= 1 + ddof
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.zeros(v.shape[1:])
        for s in range(S):
            total = total + v[s].astype(F64)
        m = total / F64(S)
        q = np.zeros(v.shape[1:])
        for s in range(S):
            d = v[s].astype(F64) - m
            q = q + d * d
        return m.astype(F32), np.sqrt(q / F64(S - ddof)).astype(F32)


# ------------------------------------------------------------------------------------------------ points
def _add(a, b):
    return a + b


def _min(a, b):
    return np.where(a < b, a, b)                                 # MinOp: a < b ? a : b


def block_reduce(values, ok, start, op):
    """values, ok: (S, M) -> (M,).  For every point, thread t folds the valid members among t, t + 256, ... in ascending order into `start`;
    then the xor butterfly 32, 16, ..., 1 inside each wave of 64 threads, then wave 0 op wave 1 op wave 2 op wave 3."""
    S, M = values.shape
    acc = np.full((THREADS, M), start, F64)
    for first in range(0, S, THREADS):
        chunk, good = values[first:first + THREADS], ok[first:first + THREADS]
        k = len(chunk)
        acc[:k] = np.where(good, op(acc[:k], chunk), acc[:k])
    acc = acc.reshape(THREADS // WAVE, WAVE, M)
    lanes = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        acc = op(acc, acc[:, lanes ^ o])
    t = acc[0, 0]
    for w in range(1, THREADS // WAVE):
        t = op(t, acc[w, 0])
    return t


def points(coords, conf=None, centre=None, min_conf=0.0, radius=1.0, ddof=0):
    """coords (S,M,2) float32, conf (S,M) float32 or None, centre (M,2) float64 or None -> (M,12) float64, column by column as the header
    lists them."""
    coords = np.asarray(coords, F32)
    S, M = coords.shape[:2]
    assert ddof in (0, 1)
    x32, y32 = coords[..., 0], coords[..., 1]
    ok = np.isfinite(x32) & np.isfinite(y32)
    c = np.zeros((S, M))
    if conf is not None:
        conf = np.asarray(conf, F32)
        ok = ok & np.isfinite(conf) & (conf >= F32(min_conf))
        c = conf.astype(F64)
    x, y, one = x32.astype(F64), y32.astype(F64), np.ones((S, M))
    r2 = F64(radius) * F64(radius)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = block_reduce(one, ok, 0.0, _add)
        sx, sy, sc = (block_reduce(a, ok, 0.0, _add) for a in (x, y, c))
        cmin = block_reduce(c, ok, np.inf, _min)
        mx, my, mc = sx / n, sy / n, sc / n
        cx, cy = (mx, my) if centre is None else (np.asarray(centre, F64)[:, 0], np.asarray(centre, F64)[:, 1])
        dx, dy, dc, ex, ey = x - mx, y - my, c - mc, x - cx, y - cy
        qxx, qyy, qxy, qcc = (block_reduce(a, ok, 0.0, _add) for a in (dx * dx, dy * dy, dx * dy, dc * dc))
        agree = block_reduce(one, ok & (ex * ex + ey * ey <= r2), 0.0, _add)
        dof = n - F64(ddof)
        vx, vy, cov = qxx / dof, qyy / dof, qxy / dof
        h, d = (vx + vy) * 0.5, (vx - vy) * 0.5
        r = np.sqrt(d * d + cov * cov)
        lo = h - r
        zero = np.zeros(M)
        cols = [n, mx, my, vx, vy, cov, h + r, np.where(lo > 0.0, lo, 0.0)]
        cols += [mc, np.sqrt(qcc / dof), cmin] if conf is not None else [zero, zero, zero]
        out = np.stack(cols + [agree], 1)
    out[n < 1 + ddof] = 0.0                                       # too few valid members: the whole row
    return out
