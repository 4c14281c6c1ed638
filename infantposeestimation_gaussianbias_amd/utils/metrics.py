"""COCOEvaluator / AverageMeter / MetricLogger with the reference's surface (utils/metrics.py:15-325).

`COCOEvaluator.update` takes what `validate()` has at hand.  When the predictions are device tensors the (B,K,3) records and the
per-instance scores come from one kernel (pk_pose_records) and ONE device->host copy per batch; numpy inputs (the reference's
calling convention) are accepted as they are -- the evaluator itself is host bookkeeping (a list of record dicts).
With an annotation file `evaluate()` reports COCO keypoint AP / AR (utils/coco_eval.py: COCOeval's arithmetic on the device, no
pycocotools); without one, the precision of greedy OKS matching against `gt_annotations=` (array form).  With `oks_nms_thr=` the records
are first rescored and thinned per image by OKS-NMS on the device (pk_pose_rescore, pk_oks_nms): the detector-box protocol."""
from collections import defaultdict
from typing import Dict, List, Optional

import numpy as np


class COCOEvaluator:
    DEFAULT_OKS_SIGMAS = np.array([0.026, 0.025, 0.025, 0.035, 0.035, 0.079, 0.079, 0.072, 0.072, 0.062, 0.062, 0.107, 0.107, 0.087,
                                   0.087, 0.089, 0.089])

    def __init__(self, ann_file: Optional[str] = None, oks_sigmas: Optional[np.ndarray] = None, num_keypoints: int = 17,
                 oks_nms_thr: Optional[float] = None, in_vis_thr: float = 0.2, soft_nms: bool = False, nms_max_dets: int = 20):
        """oks_nms_thr: None (every record is evaluated as it is), or the OKS threshold of the detector-box protocol: `evaluate()` then
        rescores every record (box score x mean of the keypoint scores above `in_vis_thr`) and removes duplicate poses per image with
        OKS-NMS -- hard, or soft (`soft_nms`, at most `nms_max_dets` poses per image) -- on the device before it computes AP."""
        self.ann_file = ann_file
        self.oks_sigmas = oks_sigmas if oks_sigmas is not None else self.DEFAULT_OKS_SIGMAS
        self.num_keypoints = num_keypoints
        self.oks_thresholds = np.linspace(0.5, 0.95, 10)
        self.oks_nms_thr, self.in_vis_thr, self.soft_nms, self.nms_max_dets = oks_nms_thr, float(in_vis_thr), bool(soft_nms), int(nms_max_dets)
        self.predictions: List[Dict] = []
        self.kept: List[Dict] = []

    def reset(self):
        self.predictions = []
        self.kept = []

    def update(self, pred_keypoints, pred_scores, image_ids, ann_ids, centers=None, scales=None, areas=None, bboxes=None, box_scores=None):
        """pred_keypoints (B,K,2) in image space, pred_scores (B,K): device tensors or numpy arrays; ids / areas / bboxes: sequences,
        arrays or tensors (utils/metrics.py:61-106: centers and scales are accepted and unused there too).  box_scores (B,): the detector's
        score of each box, stored as the record's `box_score` (None: ground-truth boxes, no such key)."""
        import torch
        if torch.is_tensor(pred_keypoints) and pred_keypoints.is_cuda:
            from .. import hipops
            rec, inst = hipops.pose_records(pred_keypoints.float(), pred_scores.float())
            rec, inst = rec.cpu().numpy().astype(np.float64), inst.cpu().numpy()
        else:
            pk, ps = np.asarray(pred_keypoints), np.asarray(pred_scores)
            rec = np.zeros((pk.shape[0], self.num_keypoints, 3))
            rec[:, :, :2], rec[:, :, 2] = pk, ps
            inst = np.array([ps[i][ps[i] > 0].mean() if (ps[i] > 0).any() else 0.0 for i in range(pk.shape[0])])
        to_list = lambda v: v.tolist() if hasattr(v, "tolist") else list(v)
        image_ids, ann_ids, areas = to_list(image_ids), to_list(ann_ids), to_list(areas)
        bboxes = bboxes.cpu().numpy() if torch.is_tensor(bboxes) else np.asarray(bboxes)
        box_scores = None if box_scores is None else to_list(box_scores)
        for i in range(rec.shape[0]):
            self.predictions.append({'image_id': int(image_ids[i]), 'ann_id': int(ann_ids[i]), 'keypoints': rec[i].flatten().tolist(),
                                     'score': float(inst[i]), 'area': float(areas[i]), 'bbox': bboxes[i].tolist()})
            if box_scores is not None:
                self.predictions[-1]['box_score'] = float(box_scores[i])

    def suppress(self) -> List[Dict]:
        """Rescoring + OKS-NMS of `self.predictions` (left untouched) -> the surviving records, copies with the updated `score`: images in
        the order of their first record, inside an image in selection order.  Two kernels over all images (pk_pose_rescore, pk_oks_nms),
        one device->host copy; the OKS uses each record's `area` and this evaluator's sigmas."""
        import torch
        from .. import _lib, hipops
        if not torch.cuda.is_available():
            raise _lib.PoseKernelError("COCOEvaluator: OKS-NMS runs on a CUDA(HIP) device; the kernels have no CPU implementation")
        recs = self.predictions
        pos_of: Dict[int, int] = {}
        pos = np.array([pos_of.setdefault(int(r['image_id']), len(pos_of)) for r in recs], np.int64)
        idx = np.argsort(pos, kind='stable')                                   # grouped by image, record order inside an image
        off = np.searchsorted(pos[idx], np.arange(len(pos_of) + 1)).astype(np.int32)
        dev = torch.device('cuda', torch.cuda.current_device())
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        kp = f64(np.array([recs[i]['keypoints'] for i in idx], np.float64).reshape(len(idx), -1, 3))
        has_box = ['box_score' in recs[i] for i in idx]
        if any(has_box) and not all(has_box):
            raise ValueError("COCOEvaluator: some records carry a box_score and some do not")
        box = f64(np.array([recs[i]['box_score'] for i in idx])) if all(has_box) and len(idx) else None
        score = hipops.pose_rescore(kp, box, self.in_vis_thr)
        sig = np.asarray(self.oks_sigmas, np.float64).reshape(-1)
        _, _, order, out_score = hipops.oks_nms(kp, f64(np.array([recs[i]['area'] for i in idx])), score, off, f64((sig * 2) ** 2),
                                                float(self.oks_nms_thr), self.in_vis_thr, self.soft_nms, self.nms_max_dets)
        both = torch.stack([order.double(), out_score]).cpu().numpy()          # local indices < 1024: exact in float64
        order_h, score_h = both[0].astype(np.int64), both[1]
        kept = []
        for i in range(len(pos_of)):
            for p in order_h[off[i]:off[i + 1]]:
                if p < 0:
                    break
                kept.append(dict(recs[idx[off[i] + p]], score=float(score_h[off[i] + p])))
        return kept

    def compute_oks(self, pred_kpts: np.ndarray, gt_kpts: np.ndarray, gt_vis: np.ndarray, area: float) -> float:
        """Object keypoint similarity of one prediction / ground-truth pair (utils/metrics.py:108-142): mean over the visible joints
        of exp(-d^2 / (2 area sigma^2 + eps)); 0 without a visible joint.  Same formula as one cell of `oks_precision`'s matrix."""
        pred_kpts, gt_kpts = np.asarray(pred_kpts, np.float64), np.asarray(gt_kpts, np.float64)
        d2 = ((pred_kpts[:, :2] - gt_kpts[:, :2]) ** 2).sum(-1)
        e = d2 / (2 * area * (np.asarray(self.oks_sigmas, np.float64) ** 2) + np.spacing(1))
        valid = np.asarray(gt_vis) > 0
        return float(np.exp(-e[valid]).sum() / valid.sum()) if valid.any() else 0.0

    def _manual_evaluate(self, gt_annotations: List[Dict]) -> Dict[str, float]:
        """The reference's fallback evaluator (utils/metrics.py:206-270): greedy score-ordered OKS matching per threshold."""
        return oks_precision(self.predictions, gt_annotations, self.oks_sigmas, self.oks_thresholds)

    def evaluate(self, gt_annotations: Optional[List[Dict]] = None) -> Dict[str, float]:
        """AP numbers for the collected records.  With an annotation file: the ten COCO keypoint numbers (AP, AP50, AP75, AP_M, AP_L,
        AR, AR50, AR75, AR_M, AR_L) of COCOKeypointEval with this evaluator's OKS sigmas; without one, `gt_annotations` (dicts with
        image_id / keypoints / area) are matched by OKS (`oks_precision`), the stand-in train.py uses to pick best.pth on loaders that
        carry no file."""
        if not self.predictions:
            return {'AP': 0.0, 'AP50': 0.0, 'AP75': 0.0}
        records = self.predictions
        if self.oks_nms_thr is not None:       # detector-box protocol: rescore, OKS-NMS per image, then AP of what survives (`self.kept`)
            records = self.kept = self.suppress()
        if self.ann_file is not None:
            from .coco_eval import COCOKeypointEval
            return COCOKeypointEval(self.ann_file, self.oks_sigmas).evaluate(records)
        if gt_annotations is None:
            raise ValueError("Either ann_file or gt_annotations must be provided")
        return oks_precision(records, gt_annotations, self.oks_sigmas, self.oks_thresholds)


def oks_precision(records, gts, sigmas, thresholds):
    """Precision of score-ordered greedy OKS matching at each threshold (the quantity utils/metrics.py:206-270 reports as "AP").

    Per image ONE (predictions x ground truths) OKS matrix is built with array arithmetic and shared by all thresholds; only the
    greedy assignment (inherently sequential: a matched ground truth leaves the pool) walks it row by row."""
    var2 = 2.0 * np.asarray(sigmas, np.float64) ** 2
    img_of_gt = np.array([g['image_id'] for g in gts])
    img_of_pr = np.array([r['image_id'] for r in records])
    gk = np.array([g['keypoints'] for g in gts], np.float64).reshape(len(gts), -1, 3)
    pk = np.array([r['keypoints'] for r in records], np.float64).reshape(len(records), -1, 3)
    g_area = np.array([g['area'] for g in gts], np.float64)
    p_score = np.array([r['score'] for r in records], np.float64)
    hits = np.zeros(len(thresholds), np.int64)
    tried = 0
    for img in dict.fromkeys(img_of_gt.tolist()):
        gi, pi = np.flatnonzero(img_of_gt == img), np.flatnonzero(img_of_pr == img)
        pi = pi[np.argsort(-p_score[pi], kind="stable")]
        tried += len(pi)
        if not len(pi):
            continue
        d2 = ((pk[pi, None, :, :2] - gk[None, gi, :, :2]) ** 2).sum(-1)                         # (P, G, K)
        vis = gk[gi, :, 2] > 0                                                                      # (G, K)
        e = np.exp(-d2 / (g_area[gi, None] * var2[None, :] + np.spacing(1))[None])
        nvis = vis.sum(-1)
        oks = np.where(nvis > 0, (e * vis[None]).sum(-1) / np.maximum(nvis, 1), 0.0)                # (P, G)
        for t, th in enumerate(thresholds):
            free = np.ones(len(gi), bool)
            for row in oks:
                cand = np.where(free, row, -1.0)
                j = int(cand.argmax())                     # first maximum, like the reference's strict '>' scan
                if cand[j] > 0 and cand[j] >= th:
                    free[j] = False
                    hits[t] += 1
    prec = hits / (tried + 1e-10)
    return {'AP': prec.mean(), 'AP50': prec[0], 'AP75': prec[5] if len(prec) > 5 else 0.0}


class AverageMeter:
    def __init__(self, name: str = '', fmt: str = ':f'):
        self.name, self.fmt = name, fmt
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val: float, n: int = 1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def __str__(self):
        return ('{name} {val' + self.fmt + '} ({avg' + self.fmt + '})').format(**self.__dict__)


class MetricLogger:
    def __init__(self, delimiter: str = '  '):
        self.meters, self.delimiter = defaultdict(AverageMeter), delimiter

    def update(self, **kwargs):
        for k, v in kwargs.items():
            self.meters[k].update(float(v))

    def __str__(self):
        return self.delimiter.join(f'{k}: {m.avg:.4f}' for k, m in self.meters.items())


# ---------------------------------------------------------------------------------------------- movement analysis and PCK
# The reference imports calculate_movement_amplitude / calculate_temporal_consistency from utils.metrics (examples/quick_start.py:159,
# visualization.py:385,441) and names PCK in both yamls, and defines none of them: the arithmetic is this project's specification (DESIGN.md
# "Movement analysis and PCK").  Everything is computed by three kernels (pk_motion_stats, pk_position_histogram, pk_pck); what is left on
# the host is bookkeeping on the one array that comes back.  Numpy input is uploaded; without a GPU these raise like every other op.
def _device_f32(x, name):
    """numpy array or tensor -> (contiguous float32 device tensor, came_as_numpy)."""
    import torch
    from .. import _lib
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            raise _lib.PoseKernelError(f"{name}: expected a CUDA(HIP) tensor or a numpy array; the kernels have no CPU implementation")
        return x.float().contiguous(), False
    if not torch.cuda.is_available():
        raise _lib.PoseKernelError(f"{name}: expected a CUDA(HIP) device; the kernels have no CPU implementation")
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device())), True


def _sequence_in(seq, confidence):
    """(T,K,2) trajectory and (T,K) / (T,K,1) confidence or None -> device tensors (1,T,K,2), (1,T,K) or None, came_as_numpy."""
    shape = tuple(seq.shape)
    if len(shape) != 3 or shape[-1] != 2:
        raise ValueError(f"sequence: expected (T, K, 2), got {shape}")
    cshape = None if confidence is None else tuple(confidence.shape)
    if cshape is not None and cshape not in (shape[:2], shape[:2] + (1,)):
        raise ValueError(f"confidence: expected {shape[:2]} or {shape[:2] + (1,)}, got {cshape}")
    coords, as_numpy = _device_f32(seq, "sequence")
    conf = None if confidence is None else _device_f32(confidence, "confidence")[0].to(coords.device).reshape(1, *shape[:2])
    return coords[None], conf, as_numpy


def _sequence_stats(seq, confidence, min_confidence):
    from .. import hipops
    coords, conf, as_numpy = _sequence_in(seq, confidence)
    return hipops.motion_stats(coords, conf, min_confidence)[0], as_numpy


def calculate_movement_amplitude(keypoints_sequence, confidence=None, min_confidence: float = 0.3):
    """Per-joint movement amplitude (K,) float64 of a (T,K,2) trajectory in pixels: the diagonal of the joint's range of motion,
    sqrt((max_x - min_x)^2 + (max_y - min_y)^2), over the frames that are finite and (with `confidence` (T,K) or (T,K,1)) at least
    `min_confidence`; 0 for a joint without such a frame.  numpy in -> numpy out, device tensor in -> device tensor out."""
    stats, as_numpy = _sequence_stats(keypoints_sequence, confidence, min_confidence)
    amp = stats[:, 5].contiguous()
    return amp.cpu().numpy() if as_numpy else amp


def _consistency(stats: np.ndarray) -> float:
    triples = float(stats[:, 10].sum())
    return float(stats[:, 9].sum()) / triples if triples > 0 else 0.0


def calculate_temporal_consistency(keypoints_sequence, confidence=None, min_confidence: float = 0.3) -> float:
    """Mean second-difference magnitude |p[t+1] - 2 p[t] + p[t-1]| over every joint and every triple of consecutive valid frames, in
    px / frame^2: lower is smoother.  0.0 when there is no triple."""
    stats, _ = _sequence_stats(keypoints_sequence, confidence, min_confidence)
    return _consistency(stats.cpu().numpy())


def movement_report(keypoints_sequence, confidence=None, flip_pairs=(), min_confidence: float = 0.3, min_movement: float = 5.0,
                    max_movement: float = 200.0, asymmetry_threshold: float = 0.2, fps: Optional[float] = None, spectrum=None, kinematics=None) -> Dict:
    """JSON-serialisable movement summary of one (T,K,2) trajectory, built from ONE (K,11) device->host copy.  Per joint: amplitude, path
    length, mean and largest speed (px / frame, or px / s with `fps`), share of valid frames, and the flag 'low' (amplitude below
    `min_movement`), 'high' (above `max_movement`) or None.  Per (left, right) pair of `flip_pairs`: ratio = |a_L - a_R| / max(a_L, a_R)
    (0 when both are 0) and asymmetric = ratio > asymmetry_threshold (examples/quick_start.py:242,249 of the reference; 5 / 200 px are
    its yaml's CLINICAL thresholds).
    spectrum=(f_min, f_max) in Hz (needs `fps`): the Hann-windowed movement spectrum of that band (`movement_spectrum`) adds, from one more
    (K,6) copy, `dominant_frequency` (Hz; None for a joint without power in the band), `peak_amplitude` (px) and `band_power` to each
    joint, `frequency_difference` (Hz, or None) to each pair and `frequency_band` to the report.  Without it the report is unchanged.
    kinematics: a dict of `kinematics_report`'s keyword arguments `angles`, `max_lag`, `entropy` (an empty one: its defaults) adds
    `report["kinematics"]`, that function's result for this trajectory, confidence, `flip_pairs`, `min_confidence` and `fps` (joint angles,
    inter-limb coordination, sample entropy: utils/kinematics.py).  Without it the report is unchanged."""
    if kinematics is not None and (not isinstance(kinematics, dict) or set(kinematics) - {"angles", "max_lag", "entropy"}):
        raise ValueError(f"movement_report: kinematics takes a dict with the keys angles, max_lag, entropy, got {kinematics!r}")
    band = None
    if spectrum is not None:
        if fps is None:
            raise ValueError("movement_report: spectrum=(f_min, f_max) is in Hz and needs fps")
        from ..configs.config import check_frequency_band
        band = check_frequency_band(spectrum, "spectrum")
        T = int(keypoints_sequence.shape[0])
        j0, F = _band_bins(float(fps), T, band[0], band[1])
    from .. import hipops
    coords, conf, _ = _sequence_in(keypoints_sequence, confidence)
    stats = hipops.motion_stats(coords, conf, min_confidence)[0]
    report = _report_from_stats(stats.cpu().numpy(), int(keypoints_sequence.shape[0]), flip_pairs, min_movement, max_movement,
                                asymmetry_threshold, fps)
    if band is not None:
        _, summary = hipops.motion_spectrum(coords, conf, min_confidence, T, j0, F, 1)
        _add_spectrum_to_report(report, summary[0].cpu().numpy(), band, T, float(fps))
    if kinematics is not None:
        from .kinematics import kinematics_report
        report["kinematics"] = kinematics_report(keypoints_sequence, confidence, flip_pairs=flip_pairs, min_confidence=min_confidence, fps=fps,
                                                 **kinematics)
    return report


def _add_spectrum_to_report(report: Dict, summary: np.ndarray, band, n_fft: int, fps: float) -> Dict:
    """The spectrum entries of `movement_report` from the (K,6) summary of pk_motion_spectrum."""
    peak = [float(summary[k, 3]) / n_fft * fps if summary[k, 3] >= 0 else None for k in range(summary.shape[0])]
    for k, joint in enumerate(report["joints"]):
        joint["dominant_frequency"] = peak[k]
        joint["peak_amplitude"] = float(np.sqrt(summary[k, 4]))
        joint["band_power"] = float(summary[k, 2])
    for pair in report["pairs"]:
        a, b = peak[pair["left"]], peak[pair["right"]]
        pair["frequency_difference"] = None if a is None or b is None else abs(a - b)
    report["frequency_band"] = [float(band[0]), float(band[1])]
    return report


def _report_from_stats(st: np.ndarray, n_frames: int, flip_pairs, min_movement, max_movement, asymmetry_threshold, fps) -> Dict:
    rate = 1.0 if fps is None else float(fps)
    joints = []
    for k in range(st.shape[0]):
        amp, steps = float(st[k, 5]), float(st[k, 7])
        joints.append({"joint": k, "amplitude": amp, "path_length": float(st[k, 6]),
                       "mean_speed": float(st[k, 6]) / steps * rate if steps > 0 else 0.0, "max_speed": float(st[k, 8]) * rate,
                       "valid_fraction": float(st[k, 0]) / n_frames if n_frames > 0 else 0.0,
                       "flag": "low" if amp < min_movement else ("high" if amp > max_movement else None)})
    pairs = []
    for left, right in flip_pairs:
        a, b = float(st[int(left), 5]), float(st[int(right), 5])
        ratio = abs(a - b) / max(a, b) if max(a, b) > 0 else 0.0
        pairs.append({"left": int(left), "right": int(right), "ratio": ratio, "asymmetric": bool(ratio > asymmetry_threshold)})
    return {"num_frames": n_frames, "fps": None if fps is None else float(fps), "speed_unit": "px/frame" if fps is None else "px/s",
            "temporal_consistency": _consistency(st), "joints": joints, "pairs": pairs}


def movement_heatmap(keypoints_sequence, image_shape, bin_size: int = 10, confidence=None, min_confidence: float = 0.3):
    """How often each joint was seen where: (K, H // bin_size, W // bin_size) int32 counts of the valid frames of a (T,K,2) trajectory,
    `image_shape` = (H, W).  Bins as plot_movement_heatmap of the reference takes them (visualization.py:248-252: np.histogram2d over
    [0, W] x [0, H] with W // 10 x H // 10 bins), rows = y.  `draw_heatmaps(img, counts.float())` overlays the result."""
    from .. import hipops
    H, W = int(image_shape[0]), int(image_shape[1])
    nbx, nby = W // int(bin_size), H // int(bin_size)
    if int(bin_size) < 1 or nbx < 1 or nby < 1:
        raise ValueError(f"movement_heatmap: bin_size {bin_size} leaves no bin in an image of {H} x {W}")
    coords, conf, as_numpy = _sequence_in(keypoints_sequence, confidence)
    counts = hipops.position_histogram(coords, np.linspace(0, W, nbx + 1), np.linspace(0, H, nby + 1), conf, min_confidence)[0]
    return counts.cpu().numpy() if as_numpy else counts


# ---------------------------------------------------------------------------------------------- movement spectrum
# How fast a joint oscillates and how much of its movement lies in a frequency band (DESIGN.md "Movement spectrum"): pk_motion_spectrum on
# the device, bin selection and unit conversion (bins -> Hz) here.
_WINDOWS = {"rect": 0, "hann": 1}


def _band_bins(fps: float, n_fft: int, f_min, f_max):
    """First bin j0 and number of bins F of the band: the bins j of 1 .. n_fft // 2 with f_min <= j / n_fft * fps <= f_max, decided on the
    very expression that `frequencies` reports.  ValueError for a band beyond the Nyquist frequency fps / 2 or one that holds no bin."""
    if not (np.isfinite(fps) and fps > 0):
        raise ValueError(f"fps must be a positive number, got {fps!r}")
    if n_fft < 2:
        raise ValueError(f"n_fft must be at least 2 (a sequence of at least 2 frames), got {n_fft}")
    if (f_min is not None and not f_min >= 0) or (f_max is not None and not f_max >= (f_min or 0)):
        raise ValueError(f"frequency band: expected 0 <= f_min <= f_max in Hz, got f_min={f_min!r}, f_max={f_max!r}")
    freq = lambda j: j / n_fft * fps
    top = n_fft // 2
    shown = f"[{0.0 if f_min is None else f_min:g}, {fps / 2 if f_max is None else f_max:g}] Hz"
    if (f_max is not None and f_max > fps / 2) or (f_min is not None and f_min > fps / 2):
        raise ValueError(f"frequency band {shown} reaches beyond the Nyquist frequency fps / 2 = {fps / 2:g} Hz")
    lo = 1 if f_min is None else min(max(int(np.ceil(f_min * n_fft / fps)), 1), top)
    while f_min is not None and lo > 1 and freq(lo - 1) >= f_min:
        lo -= 1
    while f_min is not None and lo <= top and freq(lo) < f_min:
        lo += 1
    hi = top if f_max is None else min(max(int(np.floor(f_max * n_fft / fps)), 0), top)
    while f_max is not None and hi < top and freq(hi + 1) <= f_max:
        hi += 1
    while f_max is not None and hi >= 1 and freq(hi) > f_max:
        hi -= 1
    if hi < lo:
        raise ValueError(f"frequency band {shown} holds no bin of a {n_fft}-point transform at {fps:g} fps (bins are {fps / n_fft:g} Hz apart, "
                         f"fps / 2 = {fps / 2:g} Hz)")
    return lo, hi - lo + 1


def movement_spectrum(keypoints_sequence, fps: float, confidence=None, min_confidence: float = 0.3, f_min: Optional[float] = None,
                      f_max: Optional[float] = None, n_fft: Optional[int] = None, window: str = 'hann') -> Dict:
    """Movement frequency spectrum of one (T,K,2) trajectory in pixels, recorded at `fps` frames per second (pk_motion_spectrum).  Frames
    count as for `calculate_movement_amplitude`.  The transform has `n_fft` points (default T; more zero-pads and interpolates the
    spectrum) under the periodic 'hann' window or 'rect'; the bins with f_min <= f <= f_max are computed (default: every bin from 1 to
    n_fft // 2; at most 16 384 in one call -- give a band for longer transforms).  The joint's weighted mean is removed first, so there is
    no bin 0.  ->
      frequencies (F,) Hz      (j0 + j) / n_fft * fps
      power (K,F) px^2         a linear oscillation of amplitude A px at a bin frequency has power A^2, a circle of radius R 2 R^2
      peak_frequency (K,) Hz   the bin of the largest power (NaN for a joint without power: fewer than 2 valid frames, or no movement)
      peak_amplitude (K,) px   the square root of that power
      band_power (K,) px^2     the sum over the band
      mean_frequency (K,) Hz   the power-weighted mean frequency of the band (0 without power)
    numpy in -> numpy out, device tensor in -> device tensors out (float64).  ValueError for an empty band or one beyond fps / 2."""
    from .. import hipops
    if window not in _WINDOWS:
        raise ValueError(f"window must be one of {sorted(_WINDOWS)}, got {window!r}")
    shape = tuple(keypoints_sequence.shape)
    if len(shape) != 3 or shape[-1] != 2:
        raise ValueError(f"sequence: expected (T, K, 2), got {shape}")
    N = shape[0] if n_fft is None else int(n_fft)
    j0, F = _band_bins(float(fps), N, f_min, f_max)
    coords, conf, as_numpy = _sequence_in(keypoints_sequence, confidence)
    power, summary = hipops.motion_spectrum(coords, conf, min_confidence, N, j0, F, _WINDOWS[window])
    power, summary = power[0], summary[0]
    freqs = (j0 + np.arange(F)) / N * float(fps)
    if as_numpy:
        power, summary = power.cpu().numpy(), summary.cpu().numpy()
        xp_where, nan, sqrt = np.where, np.nan, np.sqrt
    else:
        import torch
        freqs = torch.from_numpy(freqs).to(power.device)
        xp_where, nan, sqrt = torch.where, torch.full_like(summary[:, 3], float("nan")), torch.sqrt
    peak = summary[:, 3]
    return {"frequencies": freqs, "power": power, "peak_frequency": xp_where(peak >= 0, peak / N * float(fps), nan),
            "peak_amplitude": sqrt(summary[:, 4]), "band_power": summary[:, 2], "mean_frequency": summary[:, 5] / N * float(fps)}


class PCKAccumulator:
    """PCK over any number of batches: the share of keypoints within threshold x normaliser of their ground truth.  Holds the three
    device accumulators of pk_pck; `update` only launches, `compute` is the one synchronising call (one device->host copy)."""

    def __init__(self, num_keypoints: int, thresholds=(0.2,)):
        from .. import hipops
        thr = np.asarray(list(thresholds), np.float32).reshape(-1)
        if not 1 <= thr.size <= hipops.PCK_MAX_THRESHOLDS:
            raise ValueError(f"PCK: {thr.size} thresholds (1 to {hipops.PCK_MAX_THRESHOLDS})")
        self.num_keypoints, self.thresholds = int(num_keypoints), tuple(float(t) for t in thresholds)
        self._thr_host, self._thr, self._buf = thr, None, None

    def reset(self):
        self._buf = None

    def update(self, pred, gt, visible, normalizer):
        """pred, gt (N,K,2) in the same space, visible (N,K) (> 0 counts), normalizer (N,) lengths (> 0 counts): numpy or device tensors."""
        import torch
        from .. import hipops
        pred, gt = _device_f32(pred, "pred")[0], _device_f32(gt, "gt")[0]
        vis, norm = _device_f32(visible, "visible")[0], _device_f32(normalizer, "normalizer")[0]
        if pred.dim() != 3 or pred.shape[1] != self.num_keypoints:
            raise ValueError(f"pred: expected (N, {self.num_keypoints}, 2), got {tuple(pred.shape)}")
        if self._buf is None:
            self._thr = torch.from_numpy(self._thr_host).to(pred.device)
            self._buf = hipops.pck_buffers(self.num_keypoints, len(self.thresholds), pred.device)
        hipops.pck_accumulate(pred, gt, vis.to(pred.device), norm.to(pred.device), self._thr, *self._buf)

    def counts(self):
        """-> correct (n_thr,K) int64, valid (K,) int64, err_sum (K,) float64 as numpy arrays (zeros before the first update)."""
        n_thr, K = len(self.thresholds), self.num_keypoints
        if self._buf is None:
            return np.zeros((n_thr, K), np.int64), np.zeros(K, np.int64), np.zeros(K, np.float64)
        import torch
        flat = torch.cat([self._buf[0].reshape(-1).double(), self._buf[1].double(), self._buf[2]]).cpu().numpy()      # counts < 2^53: exact
        return flat[:n_thr * K].reshape(n_thr, K).astype(np.int64), flat[n_thr * K:(n_thr + 1) * K].astype(np.int64), flat[(n_thr + 1) * K:]

    def compute(self) -> Dict:
        """{'PCK@<thr>': mean over the joints with a counted pair of correct / valid, ..., 'per_joint': (n_thr,K) array (NaN for a joint
        without one), 'mean_error': mean normalised distance over all counted pairs}."""
        correct, valid, err = self.counts()
        seen = valid > 0
        per_joint = np.where(seen[None], correct / np.maximum(valid, 1)[None], np.nan)
        out = {f"PCK@{t:g}": float(per_joint[j, seen].mean()) if seen.any() else 0.0 for j, t in enumerate(self.thresholds)}
        out["per_joint"] = per_joint
        out["mean_error"] = float(err.sum() / valid.sum()) if seen.any() else 0.0
        return out


def calculate_pck(pred, gt, visible, normalizer, thresholds=(0.2,)) -> Dict:
    """PCK of one set of predictions: `PCKAccumulator(K, thresholds)` with one update."""
    acc = PCKAccumulator(int(pred.shape[1]), thresholds)
    acc.update(pred, gt, visible, normalizer)
    return acc.compute()


# ---------------------------------------------------------------------------------------------- localisation error analysis
# The numbers behind the reference's PerformanceAnalyzer (analysis/nn_quantitative_viz.py:105-252: error distribution per joint,
# confidence against accuracy, precision / recall over a confidence threshold), which it gathers in three Python loops over every
# prediction.  Here two kernels (pk_kpt_error, pk_kpt_error_quantiles: DESIGN.md "Localisation error analysis"); what is left on the
# host is arithmetic on the few arrays that come back.
def default_confidence_edges(conf_bins: int = 10) -> np.ndarray:
    """np.linspace(0, 1, conf_bins + 1) as float32 with the last edge one float32 above 1: a confidence of exactly 1.0 counts in the last
    bin (the reference's half-open bins lose it)."""
    edges = np.linspace(0, 1, int(conf_bins) + 1).astype(np.float32)
    edges[-1] = np.nextafter(np.float32(1), np.float32(np.inf))
    return edges


def _trapezoid(y, x) -> float:
    """np.trapz(y, x), written out (numpy renamed it): sum of (x[i+1] - x[i]) (y[i+1] + y[i]) / 2."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())


def _calibration(edges: np.ndarray, count: np.ndarray, hit: np.ndarray) -> Dict:
    """{edges, count, accuracy, ece} from the counts of one joint (or of all): an empty bin has accuracy 0; ece = sum_b count_b
    |accuracy_b - centre_b| / sum_b count_b (0 without a counted pair), centre_b = (edges[b] + edges[b+1]) / 2 in float64."""
    count, hit = np.asarray(count, np.int64), np.asarray(hit, np.int64)
    acc = np.where(count > 0, hit / np.maximum(count, 1), 0.0)
    e = np.asarray(edges, np.float64)
    centre = (e[:-1] + e[1:]) / 2
    total = int(count.sum())
    return {"edges": np.asarray(edges), "count": count, "accuracy": acc,
            "ece": float((count * np.abs(acc - centre)).sum() / total) if total > 0 else 0.0}


def _pr_counts(hist: np.ndarray):
    """pr_hist (..., 2, T + 1) -> tp, fp, fn (..., T) of the reference's loop at every threshold: a pair with m thresholds below its
    confidence is detected at thresholds 0 .. m - 1, so tp_i = sum_{m > i} hist[0, m], fp_i likewise from hist[1], fn_i = the correct pairs
    that are not detected."""
    hist = np.asarray(hist, np.int64)
    above = np.flip(np.cumsum(np.flip(hist, -1), -1), -1)         # above[..., m] = sum_{m' >= m}
    tp, fp = above[..., 0, 1:], above[..., 1, 1:]
    return tp, fp, above[..., 0, :1] - tp


def _precision_recall(thresholds: np.ndarray, hist: np.ndarray) -> Dict:
    """{thresholds, precision, recall, ap} of one joint (or of all): 0 where the denominator is 0, as in the reference;
    ap = -trapz(precision, recall), positive because recall falls as the threshold rises (the reference reports the negative area)."""
    tp, fp, fn = _pr_counts(hist)
    precision = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1), 0.0)
    recall = np.where(tp + fn > 0, tp / np.maximum(tp + fn, 1), 0.0)
    return {"thresholds": np.asarray(thresholds), "precision": precision, "recall": recall, "ap": -_trapezoid(precision, recall)}


def _quantile_values(order: np.ndarray, n: np.ndarray, q: np.ndarray) -> np.ndarray:
    """numpy's linear rule on the two order statistics: pos = q (n - 1), g = pos - floor(pos), value = lo + (hi - lo) g computed as
    np.percentile does (its _lerp: from the upper end when g >= 0.5).  order (K,Q,2), n (K,), q (Q,) -> (K,Q) float64; NaN where n = 0."""
    lo, hi = order[..., 0].astype(np.float64), order[..., 1].astype(np.float64)
    pos = q[None, :] * (np.maximum(n, 1)[:, None] - 1).astype(np.float64)
    g = pos - np.floor(pos)
    with np.errstate(invalid="ignore"):
        d = hi - lo
        val = np.where(g >= 0.5, hi - d * (1 - g), lo + d * g)
        val = np.where(g == 0, lo, val)                           # an exact position is the order statistic itself (inf - inf never arises)
    return np.where(n[:, None] > 0, val, np.nan)


class KeypointErrorAnalyzer:
    """Where and how the keypoints are wrong, over any number of batches: per joint the distribution of the localisation error (n, mean,
    min, max and exact quantiles), and per joint and pooled the calibration of the confidence (accuracy and count per confidence bin,
    expected calibration error) and precision / recall of "within `pixel_threshold`" over a confidence threshold with its AP.
    Holds a (K, capacity) float32 device store of every error, which grows by doubling with one device copy, and three int64 device
    counters; `update` only launches, `compute` is the one synchronising call."""

    def __init__(self, num_keypoints: int, pixel_threshold: float = 10.0, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), conf_bins=10,
                 conf_thresholds=None, capacity: int = 1024):
        """conf_bins: a number of equal bins over [0, 1] (`default_confidence_edges`) or the ascending edges themselves;
        conf_thresholds: ascending thresholds (default np.linspace(0, 1, 100), the reference's).  Edges and thresholds are rounded to
        float32 once, the type of the confidences they are compared with.  capacity: the first size of the store in samples."""
        from .. import hipops
        self.num_keypoints, self.pixel_threshold = int(num_keypoints), float(pixel_threshold)
        self.quantiles = np.asarray(list(quantiles), np.float64).reshape(-1)
        if not 1 <= self.quantiles.size <= hipops.ERR_MAX_QUANTILES or not ((self.quantiles >= 0) & (self.quantiles <= 1)).all():
            raise ValueError(f"quantiles: expected 1 to {hipops.ERR_MAX_QUANTILES} values in [0, 1], got {list(quantiles)}")
        self.edges = default_confidence_edges(conf_bins) if np.ndim(conf_bins) == 0 else np.asarray(conf_bins, np.float32).reshape(-1)
        if not 1 <= self.edges.size - 1 <= hipops.ERR_MAX_BINS or not (np.diff(self.edges) >= 0).all():
            raise ValueError(f"conf_bins: expected 1 to {hipops.ERR_MAX_BINS} bins with ascending edges, got {self.edges.size - 1}")
        thr = np.linspace(0, 1, 100) if conf_thresholds is None else np.asarray(conf_thresholds)
        self.conf_thresholds = thr.astype(np.float32).reshape(-1)
        if not 1 <= self.conf_thresholds.size <= hipops.ERR_MAX_CONF_THRESHOLDS or not (np.diff(self.conf_thresholds) >= 0).all():
            raise ValueError(f"conf_thresholds: expected 1 to {hipops.ERR_MAX_CONF_THRESHOLDS} ascending values, "
                             f"got {self.conf_thresholds.size}")
        if int(capacity) < 1:
            raise ValueError(f"capacity: expected at least 1, got {capacity}")
        self._capacity0 = int(capacity)
        self.reset()

    def reset(self):
        self._store, self._n, self._buf, self._dev = None, 0, None, None

    def update(self, pred, gt, visible, confidence=None, normalizer=None):
        """pred, gt (N,K,2) in the same space, visible (N,K) (> 0 counts), confidence (N,K) or None (the batch then enters the error
        distribution only), normalizer (N,) lengths or None (errors in the unit of the coordinates): numpy arrays or device tensors."""
        import torch
        from .. import hipops
        pred, gt, vis = _device_f32(pred, "pred")[0], _device_f32(gt, "gt")[0], _device_f32(visible, "visible")[0]
        K, dev = self.num_keypoints, pred.device
        if pred.dim() != 3 or pred.shape[1] != K:
            raise ValueError(f"pred: expected (N, {K}, 2), got {tuple(pred.shape)}")
        N = int(pred.shape[0])
        conf = None if confidence is None else _device_f32(confidence, "confidence")[0].to(dev).reshape(N, K)
        norm = None if normalizer is None else _device_f32(normalizer, "normalizer")[0].to(dev)
        if self._dev is None:
            self._dev = (torch.from_numpy(self.edges).to(dev), torch.from_numpy(self.conf_thresholds).to(dev))
            self._buf = hipops.kpt_error_buffers(K, self.edges.size - 1, self.conf_thresholds.size, dev)
        if self._store is None or self._n + N > self._store.shape[1]:
            cap = self._capacity0 if self._store is None else int(self._store.shape[1])
            while cap < self._n + N:
                cap *= 2
            grown = torch.empty(K, cap, dtype=torch.float32, device=dev)
            if self._n:
                grown[:, :self._n].copy_(self._store[:, :self._n])     # one device copy, no host round trip
            self._store = grown
        if conf is None:
            hipops.kpt_error_accumulate(pred, gt, vis.to(dev), self._store, self._n, self.pixel_threshold, normalizer=norm)
        else:
            hipops.kpt_error_accumulate(pred, gt, vis.to(dev), self._store, self._n, self.pixel_threshold, conf, norm, *self._dev, *self._buf)
        self._n += N

    def compute(self) -> Dict:
        """{'pixel_threshold', 'quantiles': the requested q,
            'joints': [{'joint', 'n', 'mean', 'min', 'max', 'quantiles': (Q,) values (numpy's linear rule; NaN like mean / min / max for a
                        joint without a counted pair), 'calibration': {edges, count, accuracy, ece}, 'pr': {thresholds, precision, recall,
                        ap}}, ...],
            'calibration', 'pr': the same two over all joints, 'ece', 'ap': the pooled ones again, 'n': all counted pairs}."""
        K, Q, nb, T = self.num_keypoints, self.quantiles.size, self.edges.size - 1, self.conf_thresholds.size
        if self._store is None or self._n == 0:
            order, summary = np.zeros((K, Q, 2), np.float32), np.zeros((K, 4))
            count = hit = np.zeros((K, nb), np.int64)
            hist = np.zeros((K, 2, T + 1), np.int64)
        else:
            import torch
            from .. import hipops
            order, summary = hipops.kpt_error_quantiles(self._store, self._n, torch.from_numpy(self.quantiles).to(self._store.device))
            counters = torch.cat([b.reshape(-1) for b in self._buf])
            order, summary, counters = order.cpu().numpy(), summary.cpu().numpy(), counters.cpu().numpy()
            count, hit = counters[:K * nb].reshape(K, nb), counters[K * nb:2 * K * nb].reshape(K, nb)
            hist = counters[2 * K * nb:].reshape(K, 2, T + 1)
        n = summary[:, 0].astype(np.int64)
        qv = _quantile_values(order, n, self.quantiles)
        joints = []
        for k in range(K):
            some = n[k] > 0
            joints.append({"joint": k, "n": int(n[k]), "mean": float(summary[k, 1] / n[k]) if some else float("nan"),
                           "min": float(summary[k, 2]) if some else float("nan"), "max": float(summary[k, 3]) if some else float("nan"),
                           "quantiles": qv[k], "calibration": _calibration(self.edges, count[k], hit[k]),
                           "pr": _precision_recall(self.conf_thresholds, hist[k])})
        calibration = _calibration(self.edges, count.sum(0), hit.sum(0))
        pr = _precision_recall(self.conf_thresholds, hist.sum(0))
        return {"pixel_threshold": self.pixel_threshold, "quantiles": self.quantiles, "n": int(n.sum()), "joints": joints,
                "calibration": calibration, "pr": pr, "ece": calibration["ece"], "ap": pr["ap"]}


def keypoint_error_report(pred, gt, visible, confidence=None, normalizer=None, **kwargs) -> Dict:
    """Error analysis of one set of predictions: `KeypointErrorAnalyzer(K, **kwargs)` with one update."""
    acc = KeypointErrorAnalyzer(int(pred.shape[1]), **kwargs)
    acc.update(pred, gt, visible, confidence, normalizer)
    return acc.compute()


def error_report_json(report: Dict) -> Dict:
    """`KeypointErrorAnalyzer.compute()` with every array as a list and every NaN as None: what `validate.py --error_report` writes."""
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, np.ndarray):
            return plain(v.tolist())
        if isinstance(v, (float, np.floating)):
            return float(v) if np.isfinite(v) else None
        if isinstance(v, np.integer):
            return int(v)
        return v
    return plain(report)
