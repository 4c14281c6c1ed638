"""COCO keypoint evaluation cases shared by test_coco_eval_host.py and test_gpu_coco_eval.py (helper module, not collected).

Hand cases A-E have results derived by hand (see each builder); `random_set` draws COCO-like files with crowds, ignored ground truths, all
three area ranges, noisy copies, false positives, score ties and (optionally) one crowded image."""
import numpy as np

COCO_SIGMAS = np.array([0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087, 0.087, 0.089,
                        0.089])
IOU_THRS = np.linspace(.5, 0.95, 10)


def pose(K, x0, y0, size, rng=None):
    """K visible joints spread over a size x size box at (x0, y0) -> (K, 3) with v = 2."""
    rng = rng or np.random.default_rng(0)
    kp = np.zeros((K, 3))
    kp[:, 0] = x0 + rng.uniform(0, size, K)
    kp[:, 1] = y0 + rng.uniform(0, size, K)
    kp[:, 2] = 2
    return kp


def gt_ann(aid, img, kp, area, bbox=None, **extra):
    kp = np.asarray(kp, np.float64)
    if bbox is None:
        x, y = kp[:, 0], kp[:, 1]
        bbox = [float(x.min()), float(y.min()), float(x.max() - x.min()), float(y.max() - y.min())]
    a = {'id': aid, 'image_id': img, 'category_id': 1, 'keypoints': kp.reshape(-1).tolist(), 'area': float(area), 'bbox': list(bbox),
         'iscrowd': 0, 'num_keypoints': int(np.count_nonzero(kp[:, 2] > 0))}
    a.update(extra)
    return a


def dataset(img_ids, anns, K=17):
    return {'images': [{'id': i, 'width': 4000, 'height': 4000, 'file_name': f'{i}.jpg'} for i in img_ids], 'annotations': anns,
            'categories': [{'id': 1, 'name': 'person', 'keypoints': [f'k{k}' for k in range(K)]}]}


def rec(img, kp, score):
    kp = np.array(kp, np.float64).copy()
    kp[:, 2] = 1.0
    return {'image_id': img, 'keypoints': kp.reshape(-1).tolist(), 'score': float(score)}


def oks_shift(gt_kp, area, sigmas, d):
    """OKS of the ground truth against itself shifted by (d, 0) (every joint visible)."""
    e = d * d / ((sigmas * 2) ** 2) / (area + np.spacing(1)) / 2
    return float(np.mean(np.exp(-e)))


def case_a():
    """1 image, 1 large ground truth, 1 detection shifted so that OKS lies in (0.70, 0.75): TP at thresholds .50-.70 (5 of 10)."""
    kp = pose(17, 100, 100, 200)
    area = 200.0 * 200.0
    lo, hi = 0.0, 200.0
    for _ in range(200):                                     # bisection on the shift for OKS = 0.725
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if oks_shift(kp, area, COCO_SIGMAS, mid) > 0.725 else (lo, mid)
    d = (lo + hi) / 2
    det = kp.copy()
    det[:, 0] += d
    want = {'AP': 0.5, 'AP50': 1.0, 'AP75': 0.0, 'AP_M': -1.0, 'AP_L': 0.5, 'AR': 0.5, 'AR50': 1.0, 'AR75': 0.0, 'AR_M': -1.0, 'AR_L': 0.5}
    return dataset([1], [gt_ann(1, 1, kp, area)]), [rec(1, det, 0.9)], want


def case_b():
    """2 large ground truths, 3 detections: .9 on gt 1, .8 far from both, .7 on gt 2 -> precision (1, 1/2, 2/3), envelope (1, 2/3, 2/3),
    recall (1/2, 1/2, 1): AP = (51 + 50 * 2/3) / 101 = 253/303 at every threshold, AR = 1."""
    g1, g2 = pose(17, 100, 100, 200, np.random.default_rng(1)), pose(17, 1000, 100, 200, np.random.default_rng(2))
    far = g1.copy()
    far[:, 1] += 2000
    ap = 253 / 303
    want = {'AP': ap, 'AP50': ap, 'AP75': ap, 'AP_M': -1.0, 'AP_L': ap, 'AR': 1.0, 'AR50': 1.0, 'AR75': 1.0, 'AR_M': -1.0, 'AR_L': 1.0}
    return (dataset([7], [gt_ann(1, 7, g1, 40000), gt_ann(2, 7, g2, 40000)]),
            [rec(7, g1, 0.9), rec(7, far, 0.8), rec(7, g2, 0.7)], want)


def case_c():
    """25 detections on one image.  Ground truths: g0, g3 normal, g1 with num_keypoints 0 (ignored), g2 crowd.  Ranked: one detection on g1
    (.995: ignored, neither TP nor FP -- as an FP it would halve the precision), three on the crowd (absorbed, ignored), one on g0 (TP), 15
    far away (FP), then five on g3 below the 20-detection cap (dropped; kept, one would be a TP and lift the recall to 1).
    -> recall 1/2 and precision 1 up to recall .5: AP = 51/101, AR = 1/2 at every threshold."""
    rng = np.random.default_rng(3)
    g = [pose(17, 100 + 600 * j, 100, 200, rng) for j in range(4)]
    anns = [gt_ann(1, 3, g[0], 40000), gt_ann(2, 3, g[1], 40000, num_keypoints=0), gt_ann(3, 3, g[2], 40000, iscrowd=1),
            gt_ann(4, 3, g[3], 40000)]
    recs = [rec(3, g[1], 0.995)] + [rec(3, g[2], s) for s in (0.994, 0.993, 0.992)] + [rec(3, g[0], 0.99)]
    for j in range(15):
        far = g[0].copy()
        far[:, 1] += 3000 + 300 * j
        recs.append(rec(3, far, 0.94 - 0.01 * j))
    recs += [rec(3, g[3], 0.1 - 0.01 * j) for j in range(5)]
    ap = 51 / 101
    want = {'AP': ap, 'AP50': ap, 'AP75': ap, 'AP_M': -1.0, 'AP_L': ap, 'AR': 0.5, 'AR50': 0.5, 'AR75': 0.5, 'AR_M': -1.0, 'AR_L': 0.5}
    return dataset([3], anns), recs, want


def case_d():
    """Two identical ground truths, one detection exactly on them: equal OKS, the later ground truth (index 1) takes the match."""
    g = pose(17, 100, 100, 200, np.random.default_rng(4))
    return dataset([5], [gt_ann(1, 5, g, 40000), gt_ann(2, 5, g, 40000)]), [rec(5, g, 0.5)]


def case_e():
    """A ground truth without visible joints (num_keypoints given as 3 so it is not ignored): OKS over all K joints of the distance to its
    box grown by its own size on each side.  Detection 0 lies inside the grown box (OKS 1), detection 1 partly outside."""
    g = pose(17, 0, 0, 1, np.random.default_rng(5))
    g[:, 2] = 0
    bbox = [100.0, 200.0, 50.0, 80.0]                        # grown box: x in [50, 200], y in [120, 360]
    area = 3000.0
    inside = np.zeros((17, 3))
    inside[:, 0], inside[:, 1] = np.linspace(60, 190, 17), np.linspace(130, 350, 17)
    out = inside.copy()
    out[::2, 0] = 20.0                                       # 30 px left of x0
    out[1::4, 1] = 400.0                                     # 40 px below y1
    dx = np.maximum(0, 50 - out[:, 0]) + np.maximum(0, out[:, 0] - 200)
    dy = np.maximum(0, 120 - out[:, 1]) + np.maximum(0, out[:, 1] - 360)
    e = (dx ** 2 + dy ** 2) / (COCO_SIGMAS * 2) ** 2 / (area + np.spacing(1)) / 2
    want_oks = [1.0, float(np.sum(np.exp(-e)) / 17)]
    return (dataset([9], [gt_ann(1, 9, g, area, bbox=bbox, num_keypoints=3)]), [rec(9, inside, 0.9), rec(9, out, 0.8)], want_oks)


def random_set(seed, n_img=300, K=17, sigmas=None, crowded=True, perfect=False, max_gt=6):
    """-> (annotation dict, records, sigmas).  Ground truths sit 450 px apart (one per column), sizes log-uniform over the three area
    ranges; ~10 % crowd, ~10 % num_keypoints 0, ~15 % of the joints invisible.  Detections: noisy copies (noise scaled to the size),
    false positives, up to 30 per image, scores rounded to 2 decimals (ties).  perfect: one record equal to every ground truth."""
    rng = np.random.default_rng(seed)
    sigmas = COCO_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)
    anns, recs, aid = [], [], 1
    img_ids = [int(i) for i in rng.permutation(np.arange(1, 3 * n_img))[:n_img] + 1000]      # ids not in file order
    crowd_img = img_ids[n_img // 2] if crowded else None
    for img in img_ids:
        G = 100 if img == crowd_img else int(rng.integers(0, max_gt + 1))
        gts = []
        for j in range(G):
            side = float(np.exp(rng.uniform(np.log(15), np.log(260))))
            kp = pose(K, 450.0 * (j % 10), 450.0 * (j // 10), side, rng)
            kp[rng.random(K) < 0.15, 2] = 0
            if rng.random() < 0.05:
                kp[:, 2] = 0
            extra = {}
            if rng.random() < 0.1:
                extra['iscrowd'] = 1
            if rng.random() < 0.1:
                extra['num_keypoints'] = 0
            a = gt_ann(aid, img, kp, side * side * rng.uniform(0.6, 1.1), bbox=[450.0 * (j % 10), 450.0 * (j // 10), side, side], **extra)
            if rng.random() < 0.1:
                a['ignore'] = 1                                # the file's own ignore key has no effect
            anns.append(a)
            gts.append((kp, side))
            aid += 1
        if perfect:
            recs += [rec(img, kp, 1.0) for kp, _ in gts]
            continue
        n_det = int(rng.integers(0, 31)) if img != crowd_img else 30
        for _ in range(n_det):
            if gts and rng.random() < 0.7:
                kp, side = gts[int(rng.integers(len(gts)))]
                det = kp.copy()
                det[:, :2] += rng.normal(0, side * rng.uniform(0.01, 0.25), (K, 2))
            else:
                det = pose(K, rng.uniform(-200, 4000), rng.uniform(-200, 4000), float(rng.uniform(10, 250)), rng)
            recs.append(rec(img, det, round(float(rng.uniform(0, 1)), 2)))
    order = rng.permutation(len(recs))                       # records arrive in any order
    return dataset(img_ids, anns, K), [recs[i] for i in order], sigmas


def near_threshold(ann, records, sigmas, tol=1e-12):
    """True if any OKS lies within `tol` of an OKS threshold (an ulp of exp could then flip a match)."""
    import cocoeval_np
    _, _, _, ious, _ = cocoeval_np.cocoeval(ann, records, sigmas)
    v = np.concatenate([np.ravel(x) for x in ious.values()] + [np.zeros(0)])
    return bool(np.any(np.abs(v[:, None] - np.minimum(IOU_THRS, 1 - 1e-10)[None, :]) <= tol))
