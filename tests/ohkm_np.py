"""Online hard keypoint mining in float64 numpy: the project's own specification of pk_ohkm_loss_fwd / _bwd (include/posekernels.h),
restated without any library code.  tests/test_ohkm_host.py holds it against the textbook torch form on the CPU; tests/test_gpu_ohkm.py
holds the kernels against it.

    L[b,k]  = (1/HW) sum_i (w[b,k] (pred - target))^2
    mask    = per sample the topk largest L: descending, a NaN before every number, equal values (and NaNs) by lower joint index
    loss    = scale / (B topk) * sum_b sum_selected L[b,k]
    d_pred  = mask * G * scale * 2 w^2 (pred - target) / (HW topk B)
"""
import numpy as np

# (B, K, H, W, topk): the smallest shapes at which each code path of the kernels can go wrong
SHAPES = [
    (2, 17, 5, 7, 8),        # HW = 35: scalar path, most threads idle
    (5, 17, 9, 3, 8),        # odd HW, unaligned map bases
    (3, 13, 40, 30, 5),      # HW = 1200: more than one trip of the strided loop
    (300, 3, 4, 4, 2),       # more samples than finalize threads, many zero-weight maps
    (2, 1, 8, 8, 1),         # K = 1
    (4, 17, 16, 12, 17),     # topk = K
    (2, 64, 6, 6, 8),        # wide K
]
SEEDS = (0, 1, 2)
U = 2.0 ** -24               # unit roundoff of float32


def cases(seed, B, K, H, W):
    """pred ~ N(0,1), target ~ U[0,1), weight drawn from {0, 0.5, 1, 1, 1}; float32, one default_rng(seed) throughout."""
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((B, K, H, W)).astype(np.float32)
    target = rng.random((B, K, H, W)).astype(np.float32)
    weight = rng.choice(np.array([0, 0.5, 1, 1, 1], np.float32), size=(B, K)).astype(np.float32)
    return pred, target, weight


def rank_order(row):
    """Indices of one sample's per-map errors in selection order: NaNs first, then descending, ties (and NaNs) by lower index."""
    return sorted(range(len(row)), key=lambda k: (0, 0.0, k) if np.isnan(row[k]) else (1, -row[k], k))


def ohkm_np(pred, target, weight, topk, scale, grad_out=1.0):
    """-> loss (float64 scalar), per_map (B,K) float64, mask (B,K) uint8, grad (like pred) float64."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    B, K = p.shape[:2]
    hw = p[0, 0].size
    w = np.ones((B, K)) if weight is None else np.asarray(weight, np.float64).reshape(B, K)
    wx = w.reshape((B, K) + (1,) * (p.ndim - 2))
    d = p - t
    per_map = ((wx * d) ** 2).reshape(B, K, hw).sum(-1) / hw
    mask = np.zeros((B, K), np.uint8)
    total = 0.0
    for b in range(B):
        for k in rank_order(per_map[b])[:topk]:
            mask[b, k] = 1
            total += per_map[b, k]
    loss = float(scale) / (B * topk) * total
    grad = mask.reshape(wx.shape) * (float(grad_out) * float(scale) * 2.0 / (hw * topk * B)) * wx * wx * d
    return loss, per_map, mask, grad


def margin(per_map, topk):
    """Smallest relative gap between the topk-th and (topk+1)-th largest error over the samples (inf when topk = K, or when both are exact
    zeros: zero-weight maps tie exactly in any arithmetic and fall to the lower index)."""
    gap = np.inf
    for row in np.asarray(per_map, np.float64):
        s = np.sort(row)[::-1]
        if topk < len(s) and not (s[topk - 1] == 0 and s[topk] == 0):
            gap = min(gap, (s[topk - 1] - s[topk]) / s[topk - 1])
    return gap


def required_margin(hw):
    """16 (HW + 4) 2^-24: sixteen times the worst-case relative error of an fp32 sum of HW non-negative terms, each a few roundings."""
    return 16 * (hw + 4) * U


_SEEDS = {}


def case_seeds(shape, weighted):
    """The three seeds of `shape`'s random cases: the first three, counting from 0, whose case satisfies the margin condition (every
    sample's topk-th and (topk+1)-th largest float64 error differ by at least required_margin, exact zeros excepted), so that the
    selection is decided by the data and not by fp32 rounding.  Decided here, in float64, before any kernel runs.  With the weights that
    is seeds 0, 1, 2 for every shape (tests/test_ohkm_host.py asserts it); without them two cases of (3, 13, 40, 30, 5) have near-ties
    (thirteen unweighted means of 1200 terms lie within a few percent of each other) and later seeds take their place."""
    key = (tuple(shape), bool(weighted))
    if key not in _SEEDS:
        B, K, H, W, topk = shape
        found, seed = [], 0
        while len(found) < len(SEEDS):
            pred, target, weight = cases(seed, B, K, H, W)
            if margin(ohkm_np(pred, target, weight if weighted else None, topk, 1.0)[1], topk) >= required_margin(H * W):
                found.append(seed)
            seed += 1
        _SEEDS[key] = tuple(found)
    return _SEEDS[key]


def exact_case():
    """(pred, target, weight, topk) with B = 4, K = 8, HW = 64, topk = 4: pred - target multiples of 0.5 with |.| <= 4, weights in {0, 1}, so
    every product, every sum of 64 of them (<= 1024, multiples of 0.25) and the division by 64 are exact in float32 in any order; the
    factor scale / (B topk) is a power of two for scale 1 and 0.5.  Sample 0: maps 1, 3, 4, 6 hold the same multiset of differences
    (permuted), and they are tied for places 3 to 6: the mask must take 1 and 3.  Sample 1: five maps tie for the top, one of them behind a
    zero weight.  Sample 2: six zero-weight maps, so two of them are selected, the lowest two.  Sample 3: no ties."""
    rng = np.random.default_rng(11)
    B, K, H, W, topk = 4, 8, 8, 8, 4
    target = (rng.integers(0, 5, (B, K, H, W)) * 0.25).astype(np.float32)
    diff = (rng.integers(-2, 3, (B, K, H, W)) * 0.5).astype(np.float32)
    weight = np.ones((B, K), np.float32)
    tied = (rng.integers(-4, 5, H * W) * 0.5).astype(np.float32)
    big = np.full(H * W, 4.0, np.float32)
    for k in (1, 3, 4, 6):
        diff[0, k] = rng.permutation(tied).reshape(H, W)
    diff[0, 2], diff[0, 7] = big.reshape(H, W), (big - 0.5).reshape(H, W)
    for k in (0, 2, 3, 5, 7):
        diff[1, k] = rng.permutation(tied).reshape(H, W)
    weight[1, 2] = 0
    weight[2, [0, 1, 3, 4, 6, 7]] = 0
    for k in range(K):
        diff[3, k] = np.float32(0.5 * (k + 1))
    return target + diff, target, weight, topk
