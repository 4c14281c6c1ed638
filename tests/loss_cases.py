"""Case table, input recipe, comparison rule and bars of the loss-unit tests (tests/test_gpu_loss_kernels.py runs the cases on the device,
tests/test_loss_host.py holds loss_np against autograd on them, holds the inputs to the conditions each case claims, and shows that the
bars can fail).  Every case is the smallest shape that reaches its regime; `regime` says which.  Seeds are fixed.

Comparison (fusion loss, spatial statistics): every map is judged alone,  stat = max_i |got - ref| / max_i |ref|  over the map.
  A map whose reference is identically zero must be identically zero.  The yardstick is the same statistic of oracle/losses.py
  evaluated in float32 on the CPU against its own float64 evaluation, floored at 2^-20; a map passes at  M x yardstick.  M (below) was
  chosen after one run on the MI355X as the smallest power of two at least twice the largest ratio seen, per output tensor; DESIGN.md
  "Loss kernels: test bars" holds the measured ratios.  Nothing is calibrated against what the kernels return.
  Pixel ties: a pixel of a skeleton pair with |sigmoid(h_i) - sigmoid(h_j)| <= 1e-5 max(...) in float64 whose two values are NOT bit
  identical is left out of the heatmap-gradient comparison (float32 may order it the other way); at most 0.1 % of a map.

Bound of the pixel loss (derived):  |got - ref| <= (k + 2) U sum|term| / count,  U = 2^-24.  k counts the fp32 roundings one term can
  pass through:  3 to form it (the difference, the product with w, the square or the smooth-L1 branch)
                 + T additions in its thread (T = trips of the grid-stride loop)
                 + 6 butterfly levels + 4 wave sums of the block reduction
                 + ceil(nb / 256) additions in the final kernel's thread + 6 + 4 again
                 + 2: the reciprocal of the count and the product with it
  so k = T + ceil(nb / 256) + 25 (pixel_k).  The backward is per element to 4 U relative: the difference, the product with the weight
  factor, the product with G / count and the reciprocal of the count; the weights of the cases carry at most 3 significant bits, so w w
  and 2 w w are exact, and the upstream gradient is 1."""
import math

import numpy as np

import loss_np as ln

U = 2.0 ** -24
FLOOR = 2.0 ** -20
LAMBDAS = (1.0, 1.0, 0.5, 0.1, 0.05, 0.05)
THRESHOLD = 0.5
SIGMA_T = 2.0
TERMS = ("heatmap", "offset", "peak", "variance", "overlap", "shape")
TIE_REL = 1e-5
TIE_SHARE = 1e-3

# M per output tensor: the margin of the device over the float32 CPU evaluation, the smallest power of two that is at least twice the
# largest ratio of one run on an MI355X and at least 1.  Largest ratios of that run: the seven values 0.61, sigma 2.39, d_heatmaps 13,
# d_offsets 6.06, d_variances 1.61, d_coords 0.97; spatial statistics mean 0.16, var 1.0, gradient 0.26 (DESIGN.md has them per term).
M = {"losses": 2, "sigma": 8, "d_hm": 32, "d_off": 16, "d_var": 4, "d_coords": 2, "mean": 1, "var": 2, "d_stats": 1}


class Fusion:
    def __init__(self, name, regime, B, K, H, W, seed, bg=-5.0, utw=True, plants=(), coords=False, claims=(), full=True):
        self.name, self.regime, self.B, self.K, self.H, self.W, self.seed, self.bg = name, regime, B, K, H, W, seed, bg
        self.utw, self.plants, self.coords, self.claims, self.full = utw, tuple(plants), coords, tuple(claims), full

    def __repr__(self):
        return self.name


# claims: "hinge" 25-75 % of the valid pairs active, "sl1" 25-75 % of |e| < 1, "mixed" a joint with an active and an inactive partner,
# "orders" both orders of S_k < S_o among the active pairs.  full=False: the one-hot upstreams only (the cases that count maps).
ALL = ("hinge", "sl1", "mixed", "orders")
FUSION = [
    Fusion("13x11 K17", "H W = 143 < 256 and no multiple of 64 (idle lanes enter block_max with -inf); hinge on and off around one joint "
           "(kin / kout over up to three partners); |e| on both sides of 1; joints in the corners (bilinear corner clamp)", 2, 17, 13, 11, 3,
           claims=ALL, plants=("w_half",)),
    Fusion("8x6 K13", "H W = 48: three of four wavefronts idle; K = 13 (pairs with joints 13..16 dropped)", 2, 13, 8, 6, 4, claims=ALL),
    Fusion("16x16 K5 twin", "H W = 256 exactly: one full trip; maps 0 and 1 of sample 1 identical bits (exact ties in min and in "
           "min(S_k, S_o)), map 3 = map 1 but for six pixels (pixel ties with S_1 < S_3)", 2, 5, 16, 16, 2, plants=("twin",), claims=("sl1",)),
    Fusion("16x17 K12", "H W = 272: a second trip of 16 lanes; K = 12: pair (11, 12) dropped, joint 11 keeps two partners; weights 0.5 "
           "and single zero weights", 2, 12, 16, 17, 3, plants=("w_half", "w_zero_some"), claims=ALL),
    Fusion("64x48 K17", "training map size, twelve trips; background -9 so that the hinge is mixed", 2, 17, 64, 48, 21, bg=-9.0, claims=ALL),
    Fusion("8x6 K21", "K > 17: joints beyond the skeleton table have no partner", 1, 21, 8, 6, 5, claims=("sl1",)),
    Fusion("8x6 K2", "K = 2: one pair", 3, 2, 8, 6, 6),
    Fusion("8x6 K1 B256", "B K = 256: k_floss_final's map loop takes exactly one trip; K = 1: no valid pair, den + 1e-8 alone",
           256, 1, 8, 6, 23, full=False),
    Fusion("8x6 K1 B257", "B K = 257: a second trip of one map", 257, 1, 8, 6, 22, full=False),
    Fusion("8x6 K17 B15", "B K = 255, B 16 = 240 pairs: the last lane of the first trip idle", 15, 17, 8, 6, 9, full=False, claims=("hinge",)),
    Fusion("8x6 K17 B17", "B 16 = 272 > 256 pairs: the pair loop takes a second trip; B K = 289", 17, 17, 8, 6, 25, full=False,
           claims=("hinge",)),
    Fusion("13x11 K5 unweighted", "use_target_weight = 0 with weights 0.5 and 0: S3 = B K, the constraint terms stay weighted", 2, 5, 13, 11, 11,
           utw=False, plants=("w_half", "w_zero_some")),
    Fusion("8x6 K5 sample off", "every weight of sample 0 is zero: its maps and pairs get exactly zero", 2, 5, 8, 6, 12, plants=("w_zero_sample",)),
    Fusion("8x6 K5 batch off", "every weight zero: S = 1e-8, den = 1e-8, all values and gradients exactly zero", 2, 5, 8, 6, 13,
           plants=("w_zero_batch",)),
    Fusion("8x6 K5 batch off unweighted", "every weight zero, use_target_weight = 0: three terms live, three exactly zero", 2, 5, 8, 6, 14,
           utw=False, plants=("w_zero_batch",)),
    Fusion("8x6 K5 coords", "coordinates handed in: interior, integer (fx = 0), exactly 0 and W - 1 / H - 1, beyond the border on each side "
           "(inx / iny, x1 clamp); map 0 all negative (R = 0), map 1 with one positive pixel of 2e-8 (QSUM = 2/3)", 2, 5, 8, 6, 15, coords=True,
           plants=("all_negative", "tiny_positive")),
    Fusion("13x11 K17 coords", "coordinates handed in on a full skeleton: d_coords next to the overlap gradient", 1, 17, 13, 11, 16, coords=True,
           claims=("sl1",)),
    Fusion("8x6 K5 special", "soft-argmax coordinates with an all-negative map and a one-pixel 2e-8 map", 1, 5, 8, 6, 17,
           plants=("all_negative", "tiny_positive")),
]


def fusion_inputs(c):
    """-> dict of float32 arrays: hm, off, var, tgt (B,K,H,W / B,K,2,H,W), w (B,K,1), gt (B,K,2, input pixels), coords or None;
    input_size = (4 W, 4 H).  Negative background + noise + one bump per joint; skeleton partners share a centre (within 0.7 px) for
    about half of the pairs; every fourth joint sits in a corner or on an edge."""
    rng = np.random.default_rng(c.seed)
    B, K, H, W = c.B, c.K, c.H, c.W
    wide = 2.0 if H * W > 1024 else 1.5
    border = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), ((W - 1) / 2, 0), (0, (H - 1) / 2), (W - 1, (H - 1) / 2), ((W - 1) / 2, H - 1)]
    ctr = np.stack([rng.uniform(1, W - 2, (B, K)), rng.uniform(1, H - 2, (B, K))], -1)
    for b in range(B):
        for k in range(3, K, 4):
            ctr[b, k] = border[(k // 4 + b) % len(border)]
        for p, (i, j) in enumerate(ln.SKELETON):
            if i < K and j < K and (p + b) % 2 == 0:
                ctr[b, j] = np.clip(ctr[b, i] + rng.uniform(-0.45, 0.45, 2), 0, (W - 1, H - 1))
    xs, ys = np.arange(W)[None, None, None, :], np.arange(H)[None, None, :, None]
    d2 = (xs - ctr[..., 0, None, None]) ** 2 + (ys - ctr[..., 1, None, None]) ** 2
    peak = rng.uniform(2.0, 4.0, (B, K, 1, 1))
    hm = c.bg + 0.3 * rng.standard_normal((B, K, H, W)) + (peak - c.bg) * np.exp(-d2 / (2 * wide * wide))
    coords = None
    if c.coords:
        coords = np.stack([rng.uniform(1, W - 2, (B, K)), rng.uniform(1, H - 2, (B, K))], -1)
        coords += 0.25 * (np.abs(coords - np.round(coords)) < 0.01)          # no accidental near-integer
        ix, iy = 3.37, 2.61                                                  # interior
        planted = [(ix, iy), (2.0, 3.0), (0.0, iy), (W - 1.0, iy), (ix, 0.0), (ix, H - 1.0), (-1.5, iy), (W + 0.5, iy), (ix, -0.75), (ix, H + 1.25)]
        flat = coords.reshape(-1, 2)
        flat[:min(len(planted), len(flat))] = planted[:len(flat)]
        coords = flat.reshape(B, K, 2).astype(np.float32)
    g_hm = (ctr if coords is None else np.clip(coords, 0, (W - 1, H - 1))) + rng.normal(0, 0.7, (B, K, 2))
    tgt = np.exp(-((xs - g_hm[..., 0, None, None]) ** 2 + (ys - g_hm[..., 1, None, None]) ** 2) / (2 * SIGMA_T ** 2))
    off = 1.3 * rng.standard_normal((B, K, 2, H, W))
    var = SIGMA_T + 0.3 + 0.5 * rng.standard_normal((B, K, H, W))          # the map mean stays clear of sigma_t
    w = np.ones((B, K, 1))
    if "w_half" in c.plants:
        w[:, 1::3] = 0.5
    if "w_zero_some" in c.plants:
        w[:, 4::5] = 0.0
    if "w_zero_sample" in c.plants:
        w[0] = 0.0
    if "w_zero_batch" in c.plants:
        w[:] = 0.0
    if "all_negative" in c.plants:
        hm[0, 0] = -np.abs(hm[0, 0]) - 0.1
    if "tiny_positive" in c.plants:
        hm[0, 1] = -np.abs(hm[0, 1]) - 0.1
        hm[0, 1, 2, 3] = 2e-8
    hm = hm.astype(np.float32)
    if "twin" in c.plants:          # sample 1: map 1 = map 0 bit for bit; map 3 = map 1 except six raised pixels (pixel ties, S_1 < S_3)
        hm[1, 1] = hm[1, 0]
        hm[1, 3] = hm[1, 1]
        hm[1, 3, 0:2, 0:3] += np.float32(0.5)
    return dict(hm=hm, off=off.astype(np.float32), var=var.astype(np.float32), tgt=tgt.astype(np.float32), w=w.astype(np.float32),
                gt=(4.0 * g_hm).astype(np.float32), coords=coords, input_size=(4.0 * W, 4.0 * H))


def upstreams(c):
    """-> [(name, lam7, g7 or None, grad_sigma or None, via)]: one-hot per term (lambda one-hot too: the term is judged alone), a random
    7-vector over all terms without and with grad_sigma, and 3 x total through hipops.fusion_loss (cases without handed-in coordinates)."""
    out = []
    for q, t in enumerate(TERMS):
        lam = np.zeros(7, np.float32)
        lam[q], lam[6] = LAMBDAS[q], THRESHOLD
        g = np.zeros(7, np.float32)
        g[q] = 1.0
        out.append((t, lam, g, None, "terms"))
    if c.full:
        rng = np.random.default_rng(100 + c.seed)
        lam = np.array(LAMBDAS + (THRESHOLD,), np.float32)
        g = rng.uniform(0.5, 1.5, 7).astype(np.float32) * np.array([1, -1, 1, 1, -1, 1, 1], np.float32)
        gs = (0.1 * rng.standard_normal((c.B, c.K))).astype(np.float32)
        out.append(("random7", lam, g, None, "terms"))
        out.append(("random7+sigma", lam, g, gs, "terms"))
        if not c.coords:
            out.append(("3total", lam, np.array([0, 0, 0, 0, 0, 0, 3], np.float32), None, "loss"))
    return out


def reference(c, x, up, defect=None):
    """loss_np on one case and upstream -> dict losses, sigma, d_hm, d_off, d_var, d_coords"""
    _, lam, g, gs, _ = up
    st = ln.fusion_forward(x["hm"], x["off"], x["var"], x["tgt"], x["w"], x["gt"], x["input_size"], SIGMA_T, lam, c.utw, x["coords"])
    d_hm, d_off, d_var, d_co = ln.fusion_backward(st, g, None, gs, defect)
    return dict(losses=st["losses"], sigma=st["sigma"], d_hm=d_hm, d_off=d_off, d_var=d_var, d_coords=d_co, state=st)


def oracle(c, x, up, dtype):
    """oracle/losses.py under autograd in `dtype` -> the same dict (numpy float64).  Handed-in coordinates enter through soft_argmax's
    place (the oracle's sample_border is differentiable in them); sigma is compute_heatmap_variance about the same coordinates."""
    import torch
    from oracle import losses as ol
    _, lam, g, gs, _ = up
    t = {k: (None if x[k] is None else torch.tensor(x[k], dtype=dtype)) for k in ("hm", "off", "var", "tgt", "w", "gt", "coords")}
    leaves = [t["hm"], t["off"], t["var"]] + ([t["coords"]] if c.coords else [])
    for a in leaves:
        a.requires_grad_(True)
    keep = ol.soft_argmax
    if c.coords:
        ol.soft_argmax = lambda hm: (t["coords"], keep(hm)[1])
    try:
        out = ol.fusion_pose_loss(t["hm"], t["off"], t["var"], t["tgt"], t["w"], t["gt"], x["input_size"], SIGMA_T,
                                  tuple(float(v) for v in lam[:6]), float(lam[6]), c.utw)
    finally:
        ol.soft_argmax = keep
    losses = torch.stack([out[n] for n in ol.NAMES])
    cc = t["coords"] if c.coords else ol.soft_argmax(t["hm"])[0]
    xs, ys = ol._grids(c.H, c.W, t["hm"])
    pos = torch.relu(t["hm"])
    Q = pos / (pos.sum((2, 3), keepdim=True) + 1e-8)
    sig = torch.sqrt((Q * ((xs - cc[..., 0, None, None]) ** 2 + (ys - cc[..., 1, None, None]) ** 2)).sum((2, 3)) + 1e-8)
    obj = (losses * torch.tensor(g, dtype=dtype)).sum()
    if gs is not None:
        obj = obj + (sig * torch.tensor(gs, dtype=dtype)).sum()
    grads = torch.autograd.grad(obj, leaves, allow_unused=True)
    gr = [np.zeros(a.shape) if v is None else v.detach().double().numpy() for a, v in zip(leaves, grads)]
    return dict(losses=losses.detach().double().numpy(), sigma=sig.detach().double().numpy(), d_hm=gr[0], d_off=gr[1], d_var=gr[2],
                d_coords=gr[3] if c.coords else None)


# ================================================================================================ comparison
def tie_mask(st):
    """(B, K, H, W) bool: pixels left out of the heatmap-gradient comparison (module docstring)"""
    s = st["s"]
    out = np.zeros(s.shape, bool)
    for i, j in st["pairs"]:
        near = (np.abs(s[:, i] - s[:, j]) <= TIE_REL * np.maximum(s[:, i], s[:, j])) & (st["hm"][:, i] != st["hm"][:, j])
        out[:, i] |= near
        out[:, j] |= near
    return out


def map_stat(got, ref, skip=None):
    """per map (the leading two axes): max |got - ref| / max |ref|; a map with ref == 0 everywhere gives 0 if got == 0 everywhere, else inf"""
    B, K = ref.shape[:2]
    g, r = np.asarray(got, np.float64).reshape(B * K, -1), np.asarray(ref, np.float64).reshape(B * K, -1)
    err = np.abs(g - r)
    if skip is not None:
        err = np.where(skip.reshape(B * K, -1), 0.0, err)
    top = np.abs(r).max(1)
    zero = top == 0
    return np.where(zero, np.where(np.abs(g).max(1) == 0, 0.0, np.inf), err.max(1) / np.where(zero, 1.0, top)).reshape(B, K)


def judge(key, got, ref, yard32, yard64, skip=None):
    """-> (largest stat / max(yardstick, floor) over the maps, its map index, passes at M[key]).  yard32 / yard64: the oracle in float32 and
    in float64 (the yardstick's error is taken against its own float64 run)."""
    if key == "losses":
        shape = (1, 7, 1)
        got, ref, yard32, yard64 = (np.asarray(a, np.float64).reshape(shape) for a in (got, ref, yard32, yard64))
    stat, yard = map_stat(got, ref, skip), map_stat(yard32, yard64, skip)
    ratio = stat / np.maximum(np.where(np.isfinite(yard), yard, 0.0), FLOOR)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at), bool(ratio[at] <= M[key])


# ================================================================================================ pixel loss
class Pixel:
    def __init__(self, name, regime, B, K, HW, weighted, seed):
        self.name, self.regime, self.B, self.K, self.HW, self.weighted, self.seed = name, regime, B, K, HW, weighted, seed

    def __repr__(self):
        return self.name

    def data(self):
        """-> pred, target (B, K, HW) float32, weight (B, K, 1) float32 or None; |pred - target| on both sides of 1; the weights are
        0, 0.5, 0.75, 1, 1.5: w w is exact in float32"""
        rng = np.random.default_rng(3000 + self.seed)
        pred = rng.standard_normal((self.B, self.K, self.HW)).astype(np.float32)
        tgt = rng.uniform(0, 1, (self.B, self.K, self.HW)).astype(np.float32)
        w = np.array([1.0, 0.5, 0.0, 0.75, 1.5], np.float32)[rng.integers(0, 5, (self.B, self.K, 1))] if self.weighted else None
        if w is not None:
            w[-1, -1] = 1.5         # the last map is where a wrapped grid takes its last trip: it must count
        return pred, tgt, w


def pixel_plan(total, cap):
    """-> (workgroups, trips of the grid-stride loop, elements in the last trip)"""
    nb = min((total + 255) // 256, cap)
    trips = (total + nb * 256 - 1) // (nb * 256)
    return nb, trips, total - (trips - 1) * nb * 256


def pixel_k(total):
    nb, trips, _ = pixel_plan(total, 1024)
    return trips + (nb + 255) // 256 + 25


PIXEL = [
    Pixel("tiny", "one workgroup, 6 elements", 1, 2, 3, True, 0),
    Pixel("HW 1", "weight[i / HW] with HW = 1: one weight per element", 5, 7, 1, True, 1),
    Pixel("HW 143", "maps that end inside a wavefront", 3, 5, 143, True, 2),
    Pixel("HW 143 unweighted", "weight == NULL", 3, 5, 143, False, 3),
    Pixel("HW 3072", "training map size, 96 workgroups", 2, 4, 3072, True, 4),
    Pixel("forward wraps", "267 264 elements = 1024 x 256 + 5 120: the forward's second trip is partly empty (20 of 1024 workgroups)",
          3, 29, 3072, True, 5),
    Pixel("backward wraps", "525 312 elements = 2048 x 256 + 1 024: the backward's second trip has 4 of 2048 workgroups; the forward's "
          "third trip 1 024 elements", 3, 57, 3072, True, 6),
    Pixel("backward wraps unweighted", "the same without weights", 3, 57, 3072, False, 7),
]
# name -> (forward plan under its cap of 1024 workgroups, backward plan under 2048): (workgroups, trips, elements of the last trip)
PIXEL_PLANS = {"forward wraps": ((1024, 2, 5120), (1044, 1, 267264)), "backward wraps": ((1024, 3, 1024), (2048, 2, 1024)),
               "backward wraps unweighted": ((1024, 3, 1024), (2048, 2, 1024))}


# ================================================================================================ spatial statistics
class Stats:
    def __init__(self, name, regime, B, K, H, W, seed):
        self.name, self.regime, self.B, self.K, self.H, self.W, self.seed = name, regime, B, K, H, W, seed

    def __repr__(self):
        return self.name

    def data(self):
        """-> hm (B, K, H, W) float32 >= 0: ReLU'd bumps; map (0,0) all zero, map (0,1) one pixel, map (0,2) of total mass 1e-8 (q = 1/2)"""
        rng = np.random.default_rng(4000 + self.seed)
        B, K, H, W = self.B, self.K, self.H, self.W
        cx, cy = rng.uniform(0, W - 1, (B, K, 1, 1)), rng.uniform(0, H - 1, (B, K, 1, 1))
        xs, ys = np.arange(W)[None, None, None, :], np.arange(H)[None, None, :, None]
        s = 1.0 if H * W <= 1024 else 2.5
        hm = np.maximum(rng.uniform(0.5, 2, (B, K, 1, 1)) * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * s * s)) - 0.05, 0)
        hm[0, 0] = 0
        hm[0, 1] = 0
        hm[0, 1, H // 2, W - 2] = 0.75
        hm[0, 2] = 0
        hm[0, 2, 1, 2], hm[0, 2, H - 2, W - 1] = 0.25e-8, 0.75e-8
        rngg = np.random.default_rng(4100 + self.seed)
        return hm.astype(np.float32), rngg.standard_normal((B, K, 2)).astype(np.float32), rngg.standard_normal((B, K, 2)).astype(np.float32)


STATS = [
    Stats("8x6", "H W = 48; a zero map (inv = 1e8, q = 0), a one-pixel map (variance 0), a map of mass 1e-8 (q = 1/2: the (1 - q) term)", 2, 3, 8, 6, 0),
    Stats("64x48", "training map size, the same special maps", 1, 4, 64, 48, 1),
]


def conditions(c, st):
    """The measurable conditions of one fusion case on the float64 reference -> dict (the host test asserts them, the table claims them)."""
    K = c.K
    ratio, v = st["ratio"], st["v"]
    valid = v > 0
    act = (ratio > THRESHOLD) & valid
    e = np.abs(st["e"][st["w3"] > 0])
    ssum = st["ssum"]
    mixed, lt, gt_ = False, 0, 0
    for b in range(c.B):
        for k in range(K):
            mine = [q for q, (i, j) in enumerate(st["pairs"]) if k in (i, j) and valid[b, q]]
            mixed |= any(act[b, q] for q in mine) and any(not act[b, q] for q in mine)
        for q, (i, j) in enumerate(st["pairs"]):
            if act[b, q] and ssum[b, i] != ssum[b, j]:
                lt += ssum[b, i] < ssum[b, j]
                gt_ += ssum[b, i] > ssum[b, j]
    gap_s = min([abs(ssum[b, i] - ssum[b, j]) / min(ssum[b, i], ssum[b, j]) for b in range(c.B) for q, (i, j) in enumerate(st["pairs"])
                 if valid[b, q] and st["hm"][b, i].tobytes() != st["hm"][b, j].tobytes()] or [math.inf])
    co = st["c"][..., 0:2] if st["ext"] else None
    return dict(active=float(act.sum() / max(valid.sum(), 1)), small_e=float((e < 1).mean()) if e.size else math.nan, mixed=bool(mixed),
                orders=(int(lt), int(gt_)), gap_r=float(np.abs(ratio - THRESHOLD)[valid].min()) if valid.any() else math.inf,
                gap_e=float(np.abs(e - 1).min()) if e.size else math.inf, gap_s=float(gap_s),
                tie_share=float(tie_mask(st).reshape(c.B * K, -1).mean(1).max()),
                gap_c=float(np.abs(co - np.round(co))[np.abs(co - np.round(co)) > 0].min()) if st["ext"] else math.inf)


def clamp_positions(x):
    """(B, K, 2) bool or None: handed-in coordinates of exactly 0, the one place where torch.clamp (gradient passes AT the bound) and
    grid_sample's border clip (gradient 0 on the bound), which the kernels and loss_np follow, take different subgradients."""
    return None if x["coords"] is None else (x["coords"] == 0)


def stats_oracle(hm, gm, gv, dtype):
    """oracle/losses.py spatial_stats under autograd -> mean, var, d_hm (numpy float64)"""
    import torch
    from oracle import losses as ol
    h = torch.tensor(hm, dtype=dtype, requires_grad=True)
    mean, var = ol.spatial_stats(h)
    (mean * torch.tensor(gm, dtype=dtype)).sum().add((var * torch.tensor(gv, dtype=dtype)).sum()).backward()
    return mean.detach().double().numpy(), var.detach().double().numpy(), h.grad.double().numpy()


def pixel_oracle(pred, tgt, w, kind, dtype):
    """oracle/losses.py for the four kinds under autograd -> loss, d_pred (numpy float64)"""
    import torch
    from oracle import losses as ol
    p = torch.tensor(pred, dtype=dtype, requires_grad=True)
    t = torch.tensor(tgt, dtype=dtype)
    ww = None if w is None else torch.tensor(w, dtype=dtype)
    p4, t4 = p[..., None], t[..., None]
    if kind == 0:
        loss = ol.keypoint_mse(p4, t4, ww)
    elif kind in (1, 2):
        loss = ol.fused_pose_loss(p4, t4, ww, "mse" if kind == 1 else "smoothl1")
    else:
        loss = ol.joints_mse_loss(p4, t4, ww if ww is not None else torch.ones(p.shape[0], p.shape[1], 1, dtype=dtype), ww is not None)
    loss.backward()
    return float(loss.detach()), p.grad.double().numpy()


def pixel_bound(total, terms):
    """(k + 2) U sum |term| / count"""
    return (pixel_k(total) + 2) * U * float(np.abs(terms).sum()) / total
