"""Independent float64 numpy restatement of COCOeval (iouType='keypoints', one category, maxDets = [20]) for the tests.

Written in COCOeval's own loop structure (evaluate -> computeOks / evaluateImg, accumulate, summarize) so that it can be read line by line
against it.  Inputs are plain: the annotation dict and the evaluator's record dicts (no category_id).  Helper module, not collected."""
import numpy as np

AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DET = 20
STAT_KEYS = ('AP', 'AP50', 'AP75', 'AP_M', 'AP_L', 'AR', 'AR50', 'AR75', 'AR_M', 'AR_L')


def _prepare(ann, records):
    img_ids = sorted(int(im['id']) for im in ann['images'])
    gts = {i: [] for i in img_ids}
    for a in ann['annotations']:
        if int(a['image_id']) in gts:
            g = dict(a)
            kp = np.asarray(g['keypoints'])
            g.setdefault('iscrowd', 0)
            g.setdefault('num_keypoints', int(np.count_nonzero(kp[2::3] > 0)))
            g['ignore'] = 'iscrowd' in g and g['iscrowd']
            g['ignore'] = (g['num_keypoints'] == 0) or g['ignore']
            gts[int(a['image_id'])].append(g)
    dts = {i: [] for i in img_ids}
    for n, r in enumerate(records):
        assert int(r['image_id']) in dts, "Results do not correspond to current coco set"
        s = r['keypoints']
        x, y = s[0::3], s[1::3]
        x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
        dts[int(r['image_id'])].append({'keypoints': s, 'score': r['score'], 'area': (x1 - x0) * (y1 - y0), 'id': n + 1, 'rec': n})
    return img_ids, gts, dts


def compute_oks(gts, dts, sigmas):
    inds = np.argsort([-d['score'] for d in dts], kind='mergesort')
    dts = [dts[i] for i in inds]
    if len(dts) > MAX_DET:
        dts = dts[0:MAX_DET]
    if len(gts) == 0 or len(dts) == 0:
        return []
    ious = np.zeros((len(dts), len(gts)))
    sigmas = np.asarray(sigmas, np.float64)
    vars = (sigmas * 2) ** 2
    k = len(sigmas)
    for j, gt in enumerate(gts):
        g = np.array(gt['keypoints'])
        xg, yg, vg = g[0::3], g[1::3], g[2::3]
        k1 = np.count_nonzero(vg > 0)
        bb = gt['bbox']
        x0, x1 = bb[0] - bb[2], bb[0] + bb[2] * 2
        y0, y1 = bb[1] - bb[3], bb[1] + bb[3] * 2
        for i, dt in enumerate(dts):
            d = np.array(dt['keypoints'])
            xd, yd = d[0::3], d[1::3]
            if k1 > 0:
                dx, dy = xd - xg, yd - yg
            else:
                z = np.zeros((k))
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars / (gt['area'] + np.spacing(1)) / 2
            if k1 > 0:
                e = e[vg > 0]
            ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
    return ious


def evaluate_img(gt, dt, ious_all, aRng, iouThrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    for g in gt:
        g['_ignore'] = 1 if (g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1])) else 0
    gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in dtind[0:MAX_DET]]
    iscrowd = [int(o['iscrowd']) for o in gt]
    ious = ious_all[:, gtind] if len(ious_all) > 0 else ious_all
    T, G, D = len(iouThrs), len(gt), len(dt)
    gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
    gtIg = np.array([g['_ignore'] for g in gt])
    dtIg = np.zeros((T, D))
    dtGt = -np.ones((T, D), np.int64)              # matched ground truth as its index in the image's file order (for the tests)
    if not len(ious) == 0:
        for tind, t in enumerate(iouThrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dtIg[tind, dind] = gtIg[m]
                dtm[tind, dind] = gt[m]['id']
                gtm[tind, m] = d['id']
                dtGt[tind, dind] = gtind[m]
    a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
    dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gtIg, 'dtIgnore': dtIg, 'dtGt': dtGt,
            'dtRec': [d['rec'] for d in dt]}


def cocoeval(ann, records, sigmas):
    """-> (stats dict, precision (T,R,A), recall (T,A), ious {image_id: (D,G)}, evalImgs [area][image])."""
    iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    img_ids, gts, dts = _prepare(ann, records)
    ious = {i: compute_oks(gts[i], dts[i], sigmas) for i in img_ids}
    evalImgs = [[evaluate_img(gts[i], dts[i], ious[i], aRng, iouThrs) for i in img_ids] for aRng in AREA_RNG]
    T, R, A = len(iouThrs), len(recThrs), len(AREA_RNG)
    precision, recall = -np.ones((T, R, A)), -np.ones((T, A))
    for a in range(A):
        E = [e for e in evalImgs[a] if e is not None]
        if len(E) == 0:
            continue
        dtScores = np.concatenate([e['dtScores'][0:MAX_DET] for e in E])
        inds = np.argsort(-dtScores, kind='mergesort')
        dtm = np.concatenate([e['dtMatches'][:, 0:MAX_DET] for e in E], axis=1)[:, inds]
        dtIg = np.concatenate([e['dtIgnore'][:, 0:MAX_DET] for e in E], axis=1)[:, inds]
        gtIg = np.concatenate([e['gtIgnore'] for e in E])
        npig = np.count_nonzero(gtIg == 0)
        if npig == 0:
            continue
        tps = np.logical_and(dtm, np.logical_not(dtIg))
        fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
        tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
        fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
        for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
            tp, fp = np.array(tp), np.array(fp)
            nd = len(tp)
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            q = np.zeros((R,))
            recall[t, a] = rc[-1] if nd else 0
            pr, q = pr.tolist(), q.tolist()
            for i in range(nd - 1, 0, -1):
                if pr[i] > pr[i - 1]:
                    pr[i - 1] = pr[i]
            inds = np.searchsorted(rc, recThrs, side='left')
            try:
                for ri, pi in enumerate(inds):
                    q[ri] = pr[pi]
            except IndexError:
                pass
            precision[t, :, a] = np.array(q)

    def mean(s):
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    t50, t75 = np.where(.5 == iouThrs)[0], np.where(.75 == iouThrs)[0]
    stats = [mean(precision[:, :, 0]), mean(precision[t50][:, :, 0]), mean(precision[t75][:, :, 0]), mean(precision[:, :, 1]),
             mean(precision[:, :, 2]), mean(recall[:, 0]), mean(recall[t50][:, 0]), mean(recall[t75][:, 0]), mean(recall[:, 1]),
             mean(recall[:, 2])]
    return dict(zip(STAT_KEYS, stats)), precision, recall, ious, evalImgs


def np_sum_order(v):
    """np.sum's order for n <= 128 float64 terms (the order pk_eval.hip's OKS sum follows), restated in Python."""
    n = len(v)
    if n < 8:
        res = 0.0
        for x in v:
            res += x
        return res
    r = [float(x) for x in v[:8]]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] += v[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in v[i:]:
        res += x
    return res
