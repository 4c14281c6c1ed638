"""COCO keypoint AP / AR without pycocotools: COCOeval(iouType='keypoints') for one category and maxDets = [20], on the device.

The host does the bookkeeping -- parse the annotation file, set the ignore flags, compute the detections' areas, check the image ids and
group both sides by image as stable index arrays -- and the HIP kernels of csrc/pk_eval.hip do the arithmetic: OKS blocks (computeOks),
the greedy matching of evaluateImg for all 3 area ranges x 10 thresholds, one global score ranking and the 30 precision / recall curves
(accumulate).  `summarize` is ten means over 30 x 101 numbers and stays on the host.  There is no CPU fallback.

Semantics are COCOeval's (DESIGN f1), with one documented deviation: an annotation without `num_keypoints` counts its joints with v > 0
(COCOeval raises a KeyError there); a missing `iscrowd` counts as 0.  Annotation id 0 is rejected (COCOeval would count its matches as
unmatched detections)."""
import json
from typing import Dict, List

import numpy as np
import torch

STAT_KEYS = ('AP', 'AP50', 'AP75', 'AP_M', 'AP_L', 'AR', 'AR50', 'AR75', 'AR_M', 'AR_L')


class COCOKeypointEval:
    AREA_RNG = ((0.0 ** 2, 1e5 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))      # all, medium, large
    MAX_DETS = 20

    def __init__(self, ann, sigmas, device=None):
        """ann: path of a COCO keypoint annotation file or the already-loaded dict; sigmas: the K per-joint OKS sigmas."""
        if not isinstance(ann, dict):
            with open(ann) as f:
                ann = json.load(f)
        cats = ann.get('categories', [])
        anns = ann.get('annotations', [])
        if len(cats) > 1 or len({a.get('category_id') for a in anns}) > 1:
            raise ValueError("COCOKeypointEval evaluates one keypoint category; the annotation file holds several")
        self.img_ids = np.array(sorted(int(im['id']) for im in ann['images']), np.int64)
        self.iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.area_rng = np.array(self.AREA_RNG, np.float64)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device()
                                                                                     if torch.cuda.is_available() else 0)
        pos_of = {int(i): p for p, i in enumerate(self.img_ids.tolist())}
        anns = [a for a in anns if int(a['image_id']) in pos_of]          # getAnnIds(imgIds=...) keeps the file's images only
        sig = np.asarray(sigmas, np.float64).reshape(-1)
        self.K = K = len(anns[0]['keypoints']) // 3 if anns else len(sig)
        if len(sig) != K:
            raise ValueError(f"{len(sig)} OKS sigmas for {K} keypoints: pass one sigma per keypoint")
        self.sigmas = sig
        self.vars = (sig * 2) ** 2
        kpt, bbox, area, flags, img_pos, ids = [], [], [], [], [], []
        for a in anns:
            kp = np.asarray(a['keypoints'], np.float64)
            if kp.size != 3 * K:
                raise ValueError(f"annotation {a.get('id')}: {kp.size} keypoint values, expected {3 * K}")
            if int(a['id']) == 0:
                raise ValueError("annotation id 0: COCOeval counts matches of such a ground truth as unmatched; renumber the file")
            crowd = int(a.get('iscrowd', 0))
            nkp = a['num_keypoints'] if 'num_keypoints' in a else int(np.count_nonzero(kp[2::3] > 0))
            kpt.append(kp.reshape(K, 3))
            bbox.append(np.asarray(a['bbox'], np.float64))
            area.append(float(a['area']))
            flags.append(int(bool(crowd or nkp == 0)) | (2 if crowd else 0))   # the file's own 'ignore' key is overwritten by COCOeval
            img_pos.append(pos_of[int(a['image_id'])])
            ids.append(int(a['id']))
        n = len(anns)
        order = np.argsort(np.asarray(img_pos, np.int64), kind='stable')
        self.gt_kpt = np.asarray(kpt, np.float64).reshape(n, K, 3)[order]
        self.gt_bbox = np.asarray(bbox, np.float64).reshape(n, 4)[order]
        self.gt_area = np.asarray(area, np.float64)[order]
        self.gt_flags = np.asarray(flags, np.int32)[order]
        self.gt_ids = np.asarray(ids, np.int64)[order]
        self.gt_off = np.searchsorted(np.asarray(img_pos, np.int64)[order], np.arange(len(self.img_ids) + 1)).astype(np.int32)
        self.precision = self.recall = None
        self.ious: Dict[int, np.ndarray] = {}

    # ---------------------------------------------------------------------------------------------------------------- host bookkeeping
    def prepare_detections(self, records: List[Dict]):
        """Records (the evaluator's dicts: image_id, keypoints (3K), score) -> arrays grouped by image (stable, record order inside an
        image): index (N,) into `records`, keypoints (N,K,3), score (N,), area (N,) = keypoint extent as loadRes computes it, dt_off."""
        K = self.K
        pos = np.searchsorted(self.img_ids, np.array([int(r['image_id']) for r in records], np.int64))
        ids = np.array([int(r['image_id']) for r in records], np.int64)
        bad = (pos >= len(self.img_ids)) | (self.img_ids[np.minimum(pos, len(self.img_ids) - 1)] != ids)
        if bad.any():
            raise ValueError(f"Results do not correspond to the annotation file: image_id {int(ids[np.argmax(bad)])} is not in its images")
        kp = np.array([r['keypoints'] for r in records], np.float64)
        if kp.ndim != 2 or kp.shape[1] != 3 * K:
            raise ValueError(f"records must carry {3 * K} keypoint values each")
        kp = kp.reshape(len(records), K, 3)
        x, y = kp[:, :, 0], kp[:, :, 1]
        area = (x.max(1) - x.min(1)) * (y.max(1) - y.min(1))
        score = np.array([r['score'] for r in records], np.float64)
        order = np.argsort(pos, kind='stable')
        dt_off = np.searchsorted(pos[order], np.arange(len(self.img_ids) + 1)).astype(np.int32)
        return order, kp[order], score[order], area[order], dt_off

    def npig(self):
        """Non-ignored ground truths per area range (host arithmetic; the device computes the same per image)."""
        ig = (self.gt_flags & 1).astype(bool)
        return np.array([np.count_nonzero(~ig & (self.gt_area >= lo) & (self.gt_area <= hi)) for lo, hi in self.area_rng])

    # ---------------------------------------------------------------------------------------------------------------- evaluation
    def evaluate(self, records: List[Dict]) -> Dict[str, float]:
        from .. import hipops
        T, R, A = len(self.iou_thrs), len(self.rec_thrs), len(self.area_rng)
        self.ious, self.dt_match, self.dt_ignore, self.slot_record, self.order = {}, None, None, np.zeros(0, np.int64), None
        if records:
            idx, kp, score, area, dt_off = self.prepare_detections(records)
        if not records or not len(self.gt_area):
            # nothing to launch: areas with non-ignored ground truth get precision / recall 0 (no detections), the others COCOeval's -1
            has = self.npig() > 0
            self.precision = np.where(has[None, None, :], 0.0, -1.0) * np.ones((T, R, A))
            self.recall = np.where(has[None, :], 0.0, -1.0) * np.ones((T, A))
            return self.summarize()
        dev = self.device
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
        n_dt, n_gt = np.diff(dt_off).astype(np.int64), np.diff(self.gt_off).astype(np.int64)
        n_cap = np.minimum(n_dt, self.MAX_DETS)
        cap_off = np.concatenate([[0], np.cumsum(n_cap)]).astype(np.int32)
        oks_off = np.concatenate([[0], np.cumsum(n_cap * n_gt)]).astype(np.int64)
        score_d, cap_off_d, gt_off_d, gt_area_d = f64(score), i32(cap_off), i32(self.gt_off), f64(self.gt_area)
        oks_off_d = torch.from_numpy(oks_off).to(dev)
        cap_idx, oks = hipops.coco_kpt_oks(f64(self.gt_kpt), f64(self.gt_bbox), gt_area_d, gt_off_d, f64(kp), score_d, i32(dt_off),
                                           f64(self.vars), cap_off_d, oks_off_d, self.MAX_DETS)
        out = hipops.coco_kpt_eval(oks, oks_off_d, gt_off_d, gt_area_d, i32(self.gt_flags), cap_off_d, cap_idx, score_d, f64(area),
                                   f64(self.area_rng), f64(self.iou_thrs), f64(self.rec_thrs))
        self.precision, self.recall = out['precision'].cpu().numpy(), out['recall'].cpu().numpy()
        self.dt_match, self.dt_ignore = out['dt_match'].cpu().numpy(), out['dt_ignore'].cpu().numpy().astype(bool)
        self.order = out['order'].cpu().numpy()
        cap = cap_idx.cpu().numpy()
        self.slot_record = idx[cap]                         # record index (into `records`) of every capped slot
        self.cap_off = cap_off
        oks_h = oks.cpu().numpy()
        for i in np.flatnonzero(n_cap * n_gt):
            self.ious[int(self.img_ids[i])] = oks_h[oks_off[i]:oks_off[i + 1]].reshape(n_cap[i], n_gt[i])
        return self.summarize()

    def summarize(self) -> Dict[str, float]:
        """COCOeval.summarize for keypoints: means of the entries > -1 of each slice (-1 if none)."""
        def mean(s):
            s = s[s > -1]
            return -1.0 if len(s) == 0 else float(np.mean(s))
        p, r = self.precision, self.recall
        t50, t75 = np.where(.5 == self.iou_thrs)[0], np.where(.75 == self.iou_thrs)[0]
        stats = [mean(p[:, :, 0]), mean(p[t50][:, :, 0]), mean(p[t75][:, :, 0]), mean(p[:, :, 1]), mean(p[:, :, 2]),
                 mean(r[:, 0]), mean(r[t50][:, 0]), mean(r[t75][:, 0]), mean(r[:, 1]), mean(r[:, 2])]
        self.stats = np.array(stats)
        return dict(zip(STAT_KEYS, stats))
