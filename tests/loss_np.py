"""The loss unit (csrc/pk_loss.hip) restated in float64 numpy from include/posekernels.h and the mathematics: the seven values of
pk_fusion_terms_fwd with the per-map sigma, the CLOSED-FORM backward of pk_fusion_terms_bwd (d_heatmaps, d_offsets, d_variances,
d_coords; the upstream 7-vector, grad_total, grad_sigma, both use_target_weight settings), the pixel losses of kinds 0 to 3 and the
spatial statistics with their backward.  tests/test_loss_host.py holds every function here against oracle/losses.py under autograd in
float64; tests/test_gpu_loss_kernels.py holds the kernels against it.

Conventions where the mathematics leaves a choice (they are the header's and grid_sample's, stated, not guessed):
  * a tie min(a, a) sends half of the gradient to either side (torch.minimum does the same), in the pixel minimum and in min(S_k, S_o);
  * a handed-in coordinate ON or beyond the border samples the clamped position and gets no gradient through the sample along that axis
    (grid_sample, padding_mode='border': its clip sets the gradient to 0 for x <= 0 and x >= W - 1).  torch.clamp, which oracle/losses.py's
    sample_border uses, passes the gradient AT the bound; the two differ at a coordinate of exactly 0 and nowhere else (at exactly W - 1
    both corners are the same pixel and the slope is 0 either way);
  * smooth-L1 has slope e for |e| < 1 and sign(e) from |e| = 1 on; relu has slope 0 at 0.

`defect=` plants ONE named error (DEFECTS); the host test shows that the bars of the device test catch each of them."""
import math

import numpy as np

SKELETON = ((0, 1), (0, 2), (1, 3), (2, 4), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12),
            (11, 12), (11, 13), (13, 15), (12, 14), (14, 16))
EPS = 1e-8
DEFECTS = {
    "no_kout": "the gradient through min(S_k, S_o) in the overlap ratio's denominator is dropped",
    "hinge_always": "the overlap hinge passes gradient for r <= threshold too",
    "tie_zero": "a tie in a minimum gets 0 instead of 1/2",
    "utw_ignored": "the backward normalises the heatmap / offset / peak terms by w / S whatever use_target_weight says",
    "qsum_one": "sum(Q) = R / (R + 1e-8) is taken as 1 in d spread / d c",
    "inx_always": "a coordinate on or beyond the border keeps its gradient through the sampled offsets",
    "sl1_slope": "smooth-L1 slope e beyond |e| = 1",
    "no_ubar": "the entropy gradient p (u - ubar) loses ubar",
    "pix_2w": "pixel kind 0 backward uses 2 w for 2 w^2",
    "no_one_minus_q": "the spatial-statistics backward drops the (1 - q) term",
}


def _f64(a):
    return np.asarray(a, np.float64)


def _sl1(e):
    a = np.abs(e)
    return np.where(a < 1, 0.5 * e * e, a - 0.5)


def _sl1_slope(e, defect=None):
    return e if defect == "sl1_slope" else np.where(np.abs(e) < 1, e, np.sign(e))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _less(a, b, defect=None):
    """d min(a, b) / d a"""
    return np.where(a < b, 1.0, np.where(a == b, 0.0 if defect == "tie_zero" else 0.5, 0.0))


def pairs_of(K):
    return [(i, j) for i, j in SKELETON if i < K and j < K]


def fusion_forward(hm, off, var, tgt, weight, gt, input_size, sigma_t, lam7, use_target_weight=True, coords=None):
    """-> state dict: 'losses' (7), 'sigma' (B, K) and everything the backward needs.  lam7 = six term weights + the overlap threshold."""
    hm, off, var, tgt, gt, lam7 = _f64(hm), _f64(off), _f64(var), _f64(tgt), _f64(gt), _f64(lam7)
    B, K, H, W = hm.shape
    n = H * W
    w = _f64(weight).reshape(B, K)
    xs, ys = np.arange(W, dtype=np.float64)[None, None, None, :], np.arange(H, dtype=np.float64)[None, None, :, None]
    P = np.exp(hm - hm.max((2, 3), keepdims=True))
    P /= P.sum((2, 3), keepdims=True)
    ext = coords is not None
    c = _f64(coords).reshape(B, K, 2) if ext else np.stack([(P * xs).sum((2, 3)), (P * ys).sum((2, 3))], -1)
    g = np.stack([gt[..., 0] * (W / input_size[0]), gt[..., 1] * (H / input_size[1])], -1)
    # bilinear sample of the two offset planes at c, border clamp
    x, y = np.clip(c[..., 0], 0, W - 1), np.clip(c[..., 1], 0, H - 1)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    flat = off.reshape(B, K, 2, n)

    def at(yi, xi):
        return np.take_along_axis(flat, np.broadcast_to((yi * W + xi)[..., None, None], (B, K, 2, 1)), 3)[..., 0]

    v00, v01, v10, v11 = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    o = v00 * (1 - fx) * (1 - fy) + v01 * fx * (1 - fy) + v10 * (1 - fx) * fy + v11 * fx * fy          # (B, K, 2)
    do_dx = (1 - fy) * (v01 - v00) + fy * (v11 - v10)
    do_dy = (1 - fx) * (v10 - v00) + fx * (v11 - v01)
    inx = ((c[..., 0] > 0) & (c[..., 0] < W - 1)).astype(np.float64)[..., None]
    iny = ((c[..., 1] > 0) & (c[..., 1] < H - 1)).astype(np.float64)[..., None]
    e = o - (g - c)
    e_hm, e_off, e_pk = ((hm - tgt) ** 2).mean((2, 3)), _sl1(e).mean(-1), ((c - g) ** 2).sum(-1)
    S = w.sum() + EPS
    w3, S3 = (w, S) if use_target_weight else (np.ones_like(w), float(B * K))
    pos = np.maximum(hm, 0)
    R = pos.sum((2, 3))
    Q = pos / (R + EPS)[..., None, None]
    r2 = (xs - c[..., 0, None, None]) ** 2 + (ys - c[..., 1, None, None]) ** 2
    spread = (Q * r2).sum((2, 3))
    sig = np.sqrt(spread + EPS)
    mv = var.mean((2, 3))
    s = _sigmoid(hm)
    ssum = s.sum((2, 3))
    pr = pairs_of(K)
    O = np.zeros((B, len(pr)))
    mn, v = np.zeros_like(O), np.zeros_like(O)
    for q, (i, j) in enumerate(pr):
        O[:, q] = np.minimum(s[:, i], s[:, j]).sum((1, 2))
        mn[:, q] = np.minimum(ssum[:, i], ssum[:, j]) + EPS
        v[:, q] = w[:, i] * w[:, j]
    ratio = O / mn if pr else O
    den = v.sum() + EPS
    lg = np.log(P + EPS)
    ent = -(P * lg).sum((2, 3))
    tent = math.log(2 * math.pi * math.e * sigma_t ** 2)
    terms = np.array([(w3 * e_hm).sum() / S3, (w3 * e_off).sum() / S3, (w3 * e_pk).sum() / S3,
                      (w * ((sig - sigma_t) ** 2 + (mv - sigma_t) ** 2)).sum() / S,
                      (np.maximum(ratio - lam7[6], 0) * v).sum() / den, (w * (ent - tent) ** 2).sum() / S])
    losses = np.concatenate([lam7[:6] * terms, [(lam7[:6] * terms).sum()]])
    return dict(losses=losses, sigma=sig, hm=hm, tgt=tgt, w=w, w3=w3, S=S, S3=S3, P=P, c=c, g=g, e=e, ext=ext, lam7=lam7, n=n,
                corners=(x0, x1, y0, y1, fx[..., 0], fy[..., 0]), do_dx=do_dx * inx, do_dy=do_dy * iny, do_raw=(do_dx, do_dy),
                pos=pos, R=R, Q=Q, r2=r2, spread=spread, mv=mv, s=s, ssum=ssum, pairs=pr, O=O, mn=mn, v=v, ratio=ratio, den=den,
                lg=lg, ent=ent, tent=tent, sigma_t=float(sigma_t), xs=xs, ys=ys, shape=(B, K, H, W))


def fusion_backward(st, grad_losses=None, grad_total=None, grad_sigma=None, defect=None):
    """Gradient of  G * sum_q (g[q] + g[6]) losses[q]  +  sum grad_sigma * sigma   (g = grad_losses or total only; G = grad_total or 1)
    -> d_heatmaps, d_offsets, d_variances, d_coords (None unless the coordinates were handed in)."""
    B, K, H, W = st["shape"]
    lam, n, hm = st["lam7"], st["n"], st["hm"]
    g7 = np.array([0, 0, 0, 0, 0, 0, 1.0]) if grad_losses is None else _f64(grad_losses)
    a = (1.0 if grad_total is None else float(grad_total)) * lam[:6] * (g7[:6] + g7[6])     # d / d (unweighted term q)
    wS = (st["w"] / st["S"])
    w3S = wS if defect == "utw_ignored" else st["w3"] / st["S3"]
    c, g, e, P = st["c"], st["g"], st["e"], st["P"]
    sig = st["sigma"]
    gs = 0.0 if grad_sigma is None else _f64(grad_sigma).reshape(B, K)
    kvar = (a[3] * wS * 2 * (sig - st["sigma_t"]) + gs) / (2 * sig)                         # d / d spread
    sl = _sl1_slope(e, defect)                                                               # (B, K, 2)
    koff = a[1] * w3S * 0.5
    do_dx, do_dy = st["do_raw"] if defect == "inx_always" else (st["do_dx"], st["do_dy"])
    qsum = np.ones_like(st["R"]) if defect == "qsum_one" else st["R"] / (st["R"] + EPS)
    qx, qy = (st["Q"] * st["xs"]).sum((2, 3)), (st["Q"] * st["ys"]).sum((2, 3))
    gcx = a[2] * w3S * 2 * (c[..., 0] - g[..., 0]) + koff * (sl[..., 0] * (do_dx[..., 0] + 1) + sl[..., 1] * do_dx[..., 1]) \
        - 2 * kvar * (qx - c[..., 0] * qsum)
    gcy = a[2] * w3S * 2 * (c[..., 1] - g[..., 1]) + koff * (sl[..., 0] * do_dy[..., 0] + sl[..., 1] * (do_dy[..., 1] + 1)) \
        - 2 * kvar * (qy - c[..., 1] * qsum)
    bc = lambda t: t[..., None, None]
    d_hm = bc(a[0] * w3S * 2 / n) * (hm - st["tgt"])
    if not st["ext"]:                                                                        # d c_x / d h_j = P_j (x_j - c_x)
        d_hm = d_hm + P * ((st["xs"] - bc(c[..., 0])) * bc(gcx) + (st["ys"] - bc(c[..., 1])) * bc(gcy))
    d_hm = d_hm + (hm > 0) * bc(kvar) * (st["r2"] - bc(st["spread"])) / bc(st["R"] + EPS)
    u = -st["lg"] - P / (P + EPS)
    ubar = 0.0 if defect == "no_ubar" else (P * u).sum((2, 3), keepdims=True)
    d_hm = d_hm + bc(a[5] * wS * 2 * (st["ent"] - st["tent"])) * P * (u - ubar)
    s, ssum = st["s"], st["ssum"]
    ds = s * (1 - s)
    for q, (i, j) in enumerate(st["pairs"]):
        on = np.ones(B) if defect == "hinge_always" else (st["ratio"][:, q] > lam[6]).astype(np.float64)
        kp = on * a[4] * st["v"][:, q] / st["den"]
        mn, O = st["mn"][:, q], st["O"][:, q]
        for k, o_ in ((i, j), (j, i)):
            through_min = 0.0 if defect == "no_kout" else -kp * _less(ssum[:, k], ssum[:, o_], defect) * O / (mn * mn)
            d_hm[:, k] += ((kp / mn)[:, None, None] * _less(s[:, k], s[:, o_], defect) + np.reshape(through_min, (-1, 1, 1))) * ds[:, k]
    x0, x1, y0, y1, fx, fy = st["corners"]
    px, py = np.arange(W)[None, None, None, :], np.arange(H)[None, None, :, None]
    wx = (px == bc(x0)) * bc(1 - fx) + (px == bc(x1)) * bc(fx)
    wy = (py == bc(y0)) * bc(1 - fy) + (py == bc(y1)) * bc(fy)
    d_off = (bc(koff) * wx * wy)[:, :, None] * sl[..., None, None]
    d_var = np.broadcast_to(bc(a[3] * wS * 2 * (st["mv"] - st["sigma_t"]) / n), hm.shape).copy()
    return d_hm, d_off, d_var, (np.stack([gcx, gcy], -1) if st["ext"] else None)


# ================================================================================================ pixel losses
def pixel_terms(pred, tgt, weight, kind):
    """-> the B*K*HW terms whose mean is the loss (float64, shape (B, K, HW))"""
    B, K = pred.shape[:2]
    d = (_f64(pred) - _f64(tgt)).reshape(B, K, -1)
    w = np.ones((B, K, 1)) if weight is None else _f64(weight).reshape(B, K, 1)
    return [(d * w) ** 2, w * d * d, w * _sl1(d), 0.5 * (d * w) ** 2][kind]


def pixel_loss(pred, tgt, weight, kind):
    return float(pixel_terms(pred, tgt, weight, kind).mean())


def pixel_loss_bwd(pred, tgt, weight, kind, grad_out=1.0, defect=None):
    B, K = pred.shape[:2]
    d = (_f64(pred) - _f64(tgt)).reshape(B, K, -1)
    w = np.ones((B, K, 1)) if weight is None else _f64(weight).reshape(B, K, 1)
    g = [2 * (w if defect == "pix_2w" else w * w) * d, 2 * w * d, w * _sl1_slope(d), w * w * d][kind]
    return (float(grad_out) / d.size * g).reshape(np.shape(pred))


# ================================================================================================ spatial statistics
def spatial_stats(hm):
    """-> mean (B, K, 2), var (B, K, 2) of hm / (sum hm + 1e-8)"""
    hm = _f64(hm)
    H, W = hm.shape[2:]
    xs, ys = np.arange(W, dtype=np.float64)[None, None, None, :], np.arange(H, dtype=np.float64)[None, None, :, None]
    p = hm / (hm.sum((2, 3), keepdims=True) + EPS)
    mx, my = (p * xs).sum((2, 3)), (p * ys).sum((2, 3))
    vx, vy = (p * (xs - mx[..., None, None]) ** 2).sum((2, 3)), (p * (ys - my[..., None, None]) ** 2).sum((2, 3))
    return np.stack([mx, my], -1), np.stack([vx, vy], -1)


def spatial_stats_bwd(hm, grad_mean, grad_var, defect=None):
    """With S = sum h, inv = 1 / (S + 1e-8), q = S inv:  d m / d h_j = inv (x_j - m);  d v / d h_j = inv ((x_j - m)^2 - v) - 2 inv (x_j - m) m (1 - q):
    the last term is sum_i p_i (x_i - m) = m (1 - q), which is not 0 because the p_i do not sum to 1."""
    hm, gm, gv = _f64(hm), _f64(grad_mean), _f64(grad_var)
    H, W = hm.shape[2:]
    mean, var = spatial_stats(hm)
    S = hm.sum((2, 3))
    inv = 1.0 / (S + EPS)
    omq = np.zeros_like(S) if defect == "no_one_minus_q" else 1.0 - S * inv
    out = np.zeros_like(hm)
    for ax, coord in ((0, np.arange(W, dtype=np.float64)[None, None, None, :]), (1, np.arange(H, dtype=np.float64)[None, None, :, None])):
        m, v = mean[..., ax, None, None], var[..., ax, None, None]
        d = coord - m
        out = out + gm[..., ax, None, None] * d + gv[..., ax, None, None] * (d * d - v - 2 * d * m * omq[..., None, None])
    return out * inv[..., None, None]
