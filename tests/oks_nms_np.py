"""Independent numpy restatement of pose rescoring and OKS-NMS ("Detector boxes and OKS-NMS"; include/posekernels.h), and
the generator of the test inputs.  Written from the specification, loop by loop: one Python loop over the images, one over the links of the
greedy chain, one over the joints k ascending (the arithmetic of one joint is done for all candidate poses at once: adding an exact 0.0 for
a joint that does not count leaves a sum as it is, so every sum is still the k-ascending one).

Besides the result each function returns its MARGIN: how close the data came to a decision that one ulp could flip --
  hard mode: the smallest |oks - thr| among the comparisons made;
  soft mode: the smallest relative gap between the two highest current scores at a selection (exact ties excluded: those resolve by index).
A test asserts the margin before it demands exact equality of keep / order."""
import math

import numpy as np

EPS = 2.220446049250313e-16
COCO_SIGMAS = np.array([0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087, 0.087, 0.089, 0.089])


def rescore_np(kpt, box_score, in_vis_thr):
    """(N,K,3), (N,) or None -> (N,): box score x mean of the keypoint scores > in_vis_thr (sum over k ascending), 0 without one."""
    kpt = np.asarray(kpt, np.float64)
    out = np.zeros(kpt.shape[0])
    for i in range(kpt.shape[0]):
        total, cnt = 0.0, 0
        for k in range(kpt.shape[1]):
            s = float(kpt[i, k, 2])
            if s > in_vis_thr:
                total += s
                cnt += 1
        mean = total / cnt if cnt else 0.0
        out[i] = (1.0 if box_score is None else float(box_score[i])) * mean
    return out


def oks_to(sel, area_sel, others, area_others, vars_, in_vis_thr):
    """OKS of pose `sel` (K,3) to each of `others` (M,K,3) -> (M,)."""
    M, K = others.shape[0], others.shape[1]
    denom = (area_sel + area_others) / 2.0 + EPS
    total, cnt = np.zeros(M), np.zeros(M, np.int64)
    for k in range(K):
        both = (others[:, k, 2] > in_vis_thr) & bool(sel[k, 2] > in_vis_thr)
        dx, dy = sel[k, 0] - others[:, k, 0], sel[k, 1] - others[:, k, 1]
        e = (dx * dx + dy * dy) / vars_[k] / denom / 2.0
        total = total + np.where(both, np.exp(-e), 0.0)
        cnt += both
    return np.where(cnt > 0, total / np.maximum(cnt, 1), 0.0)


def _rank_key(s, j):
    """Sort key of descending score, NaN last, ties to the lower index (-0 == +0)."""
    return (1, 0.0, j) if math.isnan(s) else (0, -s, j)


def oks_nms_np(kpt, area, score, off, vars_, thr, in_vis_thr, soft=False, max_dets=20):
    """-> keep (N,) uint8, n_keep (n_img,) int32, order (N,) int32, out_score (N,) float64, margin (float, inf when nothing was compared)."""
    kpt, area, score = np.asarray(kpt, np.float64), np.asarray(area, np.float64), np.asarray(score, np.float64)
    vars_ = np.asarray(vars_, np.float64)
    N, n_img = kpt.shape[0], len(off) - 1
    keep, order, out_score = np.zeros(N, np.uint8), np.full(N, -1, np.int32), np.zeros(N)
    n_keep = np.zeros(n_img, np.int32)
    margin = math.inf
    if soft and not thr > 0:
        raise ValueError("soft mode needs thr > 0")
    for img in range(n_img):
        d0, n = int(off[img]), int(off[img + 1] - off[img])
        kp, ar, cur = kpt[d0:d0 + n], area[d0:d0 + n], score[d0:d0 + n].copy()
        picked = []
        if not soft:
            visit = sorted(range(n), key=lambda j: _rank_key(float(cur[j]), j))
            alive = np.ones(n, bool)
            for pos, p in enumerate(visit):
                if not alive[p]:
                    continue
                picked.append(p)
                later = np.array([c for c in visit[pos + 1:] if alive[c]], np.int64)
                if later.size:
                    o = oks_to(kp[p], ar[p], kp[later], ar[later], vars_, in_vis_thr)
                    margin = min(margin, float(np.nanmin(np.abs(o - thr))) if not np.isnan(o).all() else math.inf)
                    alive[later[o > thr]] = False
        else:
            remaining = list(range(n))
            while remaining and len(picked) < max_dets:
                ranked = sorted(remaining, key=lambda j: _rank_key(float(cur[j]), j))
                p = ranked[0]
                if len(ranked) > 1:
                    s1, s2 = float(cur[p]), float(cur[ranked[1]])
                    if not (math.isnan(s1) or math.isnan(s2)) and s1 != s2:
                        margin = min(margin, (s1 - s2) / abs(s1))
                picked.append(p)
                remaining.remove(p)
                if remaining:
                    rest = np.array(remaining, np.int64)
                    o = oks_to(kp[p], ar[p], kp[rest], ar[rest], vars_, in_vis_thr)
                    cur[rest] = cur[rest] * np.exp(-(o * o) / thr)
        n_keep[img] = len(picked)
        for r, p in enumerate(picked):
            keep[d0 + p] = 1
            order[d0 + r] = p
            out_score[d0 + p] = cur[p]
    return keep, n_keep, order, out_score, margin


# ---------------------------------------------------------------------------------------------------------------- test inputs
def sigmas_for(K, rng):
    return COCO_SIGMAS.copy() if K == 17 else rng.uniform(0.025, 0.107, K)


def make_image(n, K, sigmas, rng, tie):
    """n detections of one image: about n / 4 base poses in boxes of side 60-200 px, each detection = a base pose + Gaussian jitter
    j sqrt(area) 2 sigma_k per coordinate with j from {0, 0.3, 1, 3}; keypoint scores U(0, 1), pose scores U(0.05, 1) -- all distinct, then
    with tie=True exactly one pair made equal."""
    nb = max(1, int(round(n / 4)))
    side = rng.uniform(60.0, 200.0, nb)
    corner = rng.uniform(0.0, 800.0, (nb, 2))
    base = corner[:, None, :] + rng.uniform(0.0, 1.0, (nb, K, 2)) * side[:, None, None]
    b = rng.permutation(n) % nb                  # clusters of 4 (the last ones may hold fewer), scattered over the indices
    j = rng.choice(np.array([0.0, 0.3, 1.0, 3.0]), n)
    area = side[b] ** 2
    kpt = np.zeros((n, K, 3))
    kpt[:, :, :2] = base[b] + rng.standard_normal((n, K, 2)) * (j * np.sqrt(area))[:, None, None] * (2.0 * sigmas)[None, :, None]
    kpt[:, :, 2] = rng.uniform(0.0, 1.0, (n, K))
    score = rng.uniform(0.05, 1.0, n)
    while len(set(score.tolist())) != n:
        score = rng.uniform(0.05, 1.0, n)
    if tie and n >= 2:
        a, c = rng.choice(n, 2, replace=False)
        score[c] = score[a]
    return kpt, area, score


def make_batch(counts, K, seed, tie):
    """CSR batch of images with the given pose counts -> kpt (N,K,3), area (N,), score (N,), off (n_img+1,) int32, vars (K,)."""
    rng = np.random.default_rng(seed)
    sig = sigmas_for(K, rng)
    parts = [make_image(n, K, sig, rng, tie) for n in counts]
    kpt = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, K, 3))
    area, score = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return kpt.reshape(-1, K, 3), area, score, off, (2.0 * sig) ** 2
