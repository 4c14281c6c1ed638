"""Post-processing (drop-in for the reference's utils/postprocess.py hot-path functions), all on device:
the reference's Python B x K loops with .item() become one kernel launch each."""
import torch

from .. import hipops


def get_max_preds(batch_heatmaps):
    """-> preds (B,K,2) float32 (x,y), maxvals (B,K,1) (postprocess.py:10-34)."""
    _, mv, co = hipops.argmax_decode(batch_heatmaps.float(), 0)
    return co, mv.unsqueeze(-1)


def get_max_preds_with_subpixel(batch_heatmaps):
    """Argmax + Taylor sub-pixel step (postprocess.py:37-75)."""
    _, mv, co = hipops.argmax_decode(batch_heatmaps.float(), 2)
    return co, mv.unsqueeze(-1)


def get_max_preds_unbiased(batch_heatmaps, kernel=11):
    """Argmax + the unbiased (distribution-aware) step: one Newton step on the logarithm of the map smoothed with a `kernel`-tap Gaussian
    (pk_unbiased_decode; where the step is not taken the integer argmax stands).  -> preds (B,K,2), maxvals (B,K,1) like its siblings."""
    _, mv, co, _ = hipops.unbiased_decode(batch_heatmaps.float(), kernel)
    return co, mv.unsqueeze(-1)


def fused_decode(heatmaps, regression_coords=None, centers=None, scales=None, alpha=0.5):
    """postprocess.py:78-135 incl. its quirks (hard-coded 256 image size; the alpha blend is overwritten by the
    confidence-adaptive blend, so `alpha` has no effect — kept for signature parity)."""
    hp, mv = get_max_preds_with_subpixel(heatmaps)
    H, W = heatmaps.shape[2:]
    sx, sy = (256 / W, 256 / H) if (centers is not None and scales is not None) else (1.0, 1.0)
    reg_scale = 1.0
    if regression_coords is not None:
        regression_coords = regression_coords.float()
        if float(regression_coords.max()) <= 1.0:     # one host sync, exactly where the reference has one
            reg_scale = 256.0
    return hipops.fused_blend(hp, mv.squeeze(-1) if regression_coords is not None else None, regression_coords, sx, sy, reg_scale), mv


def coordinate_refinement(heatmaps, initial_coords, window_size=5):
    return hipops.window_refine(heatmaps.float(), initial_coords.float(), window_size)


def filter_low_confidence(preds, maxvals, threshold=0.3):
    mask = (maxvals > threshold).float()
    return preds * mask, mask


def temporal_smoothing(coords_sequence, window_size=5, method="gaussian"):
    """Reference signature (utils/postprocess.py:187-223): (T,K,2) trajectories smoothed along T on the device (one launch
    instead of 2K numpy round trips).  The weights are built exactly as the reference builds them (float64, one-sided
    'gaussian' or uniform); even windows raise like the reference's shape mismatch does."""
    import numpy as np
    if method == "gaussian":
        sigma = window_size / 3.0
        kernel = np.exp(-np.arange(window_size) ** 2 / (2 * sigma ** 2))
        kernel = kernel / kernel.sum()
    else:
        kernel = np.ones(window_size) / window_size
    return hipops.temporal_smooth(coords_sequence, kernel)


def nms_pose(preds, maxvals, distance_threshold=5.0):
    """Reference signature (utils/postprocess.py:241-267): -> (preds * keep, keep (B,K,1) bool)."""
    return hipops.nms_pose(preds, maxvals, distance_threshold)


def _oks_nms(kpts, scores, areas, thr, sigmas, in_vis_thr, offsets, soft, max_dets):
    """Shared body of `oks_nms` / `soft_oks_nms`: numpy arrays are uploaded (and numpy comes back), device tensors are used as they are.
    -> kept global indices (int64; images in order, selection order inside an image), their scores."""
    import numpy as np
    as_numpy = not torch.is_tensor(kpts)
    if as_numpy and not torch.cuda.is_available():
        from .. import _lib
        raise _lib.PoseKernelError("oks_nms: expected a CUDA(HIP) device; the kernels have no CPU implementation")
    dev = kpts.device if not as_numpy else torch.device("cuda", torch.cuda.current_device())
    f64 = lambda v: (v.to(torch.float64) if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev))
    kp = f64(kpts)
    if kp.dim() != 3 or kp.shape[-1] != 3:
        raise ValueError(f"kpts: expected (N, K, 3) rows [x, y, score], got {tuple(kp.shape)}")
    N, K = int(kp.shape[0]), int(kp.shape[1])
    if sigmas is None:
        from .metrics import COCOEvaluator
        sigmas = COCOEvaluator.DEFAULT_OKS_SIGMAS
        if K != len(sigmas):
            raise ValueError(f"oks_nms: pass one OKS sigma per keypoint (the default holds the {len(sigmas)} COCO sigmas, got K = {K})")
    sig = np.asarray(sigmas.cpu() if torch.is_tensor(sigmas) else sigmas, np.float64).reshape(-1)
    if sig.size != K:
        raise ValueError(f"oks_nms: {sig.size} OKS sigmas for {K} keypoints")
    if offsets is None:
        off = np.array([0, N], np.int32)
    else:
        off = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets)
        if off.ndim != 1 or off.size < 2 or (off != off.astype(np.int32)).any():
            raise ValueError("offsets: expected n_img + 1 integer CSR offsets")
        off = off.astype(np.int32)
    _, n_keep, order, out_score = hipops.oks_nms(kp, f64(areas).reshape(-1), f64(scores).reshape(-1), off, f64((sig * 2) ** 2), thr,
                                                 in_vis_thr, soft, max_dets)
    base = torch.repeat_interleave(torch.from_numpy(off[:-1].astype(np.int64)), torch.from_numpy(np.diff(off).astype(np.int64))).to(dev)
    sel = order >= 0                                   # per image the kept slots come first, so masking preserves the selection order
    idx = (order.to(torch.int64) + base)[sel]
    sc = out_score[idx]
    return (idx.cpu().numpy(), sc.cpu().numpy()) if as_numpy else (idx, sc)


def oks_nms(kpts, scores, areas, thr=0.9, sigmas=None, in_vis_thr=0.2, offsets=None):
    """Hard OKS-NMS of the poses of one image, or of a CSR batch of images (`offsets`: n_img + 1 ascending offsets into the N poses), on
    the device (pk_oks_nms).  kpts (N,K,3) rows [x, y, keypoint score], scores (N,), areas (N,); sigmas: the K OKS sigmas (default: COCO's 17).
    Per image the poses are visited by descending score (ties to the lower index); a visited pose that is still alive is kept and removes
    every later pose whose OKS to it exceeds `thr`; a joint counts in the OKS when both keypoint scores exceed `in_vis_thr`.
    -> the kept indices (int64), image by image, in selection order.  At most 1024 poses per image."""
    return _oks_nms(kpts, scores, areas, thr, sigmas, in_vis_thr, offsets, False, 0)[0]


def soft_oks_nms(kpts, scores, areas, thr=0.9, sigmas=None, in_vis_thr=0.2, offsets=None, max_dets=20):
    """Soft OKS-NMS: per image, until `max_dets` poses are kept, the remaining pose with the highest current score is selected and every
    remaining score is multiplied by exp(-oks^2 / thr).  -> (kept indices, their scores at selection)."""
    return _oks_nms(kpts, scores, areas, thr, sigmas, in_vis_thr, offsets, True, max_dets)


def transform_preds(coords, center, scale, output_size, input_size=[256, 256]):
    return hipops.affine_coords(coords.float(), center.float().to(coords.device), scale.float().to(coords.device),
                                1.0 / input_size[0], 1.0 / input_size[1])


def postprocess_predictions(outputs, batch_meta, config):
    heatmaps = outputs['heatmaps']
    alpha = config.TEST.FUSION_ALPHA if hasattr(config.TEST, 'FUSION_ALPHA') else 0.5
    preds, maxvals = fused_decode(heatmaps, outputs.get('coords', None), batch_meta.get('center'), batch_meta.get('scale'), alpha)
    preds = coordinate_refinement(heatmaps, preds)
    preds, mask = filter_low_confidence(preds, maxvals, threshold=0.3)
    if 'center' in batch_meta and 'scale' in batch_meta:
        preds = transform_preds(preds, batch_meta['center'], batch_meta['scale'], output_size=[640, 480])
    return {'preds': preds, 'maxvals': maxvals, 'mask': mask}


def heatmap_to_image_coords(pred_keypoints, center, scale, input_size, heatmap_size):
    """train.py:286-303 / validate.py:100-117 as one launch: heat-px -> input-px -> original image (no Python B x K loop)."""
    mul_x = (input_size[0] / heatmap_size[0]) / input_size[0]
    mul_y = (input_size[1] / heatmap_size[1]) / input_size[1]
    return hipops.affine_coords(pred_keypoints.float(), center.float().to(pred_keypoints.device),
                                scale.float().to(pred_keypoints.device), mul_x, mul_y)
