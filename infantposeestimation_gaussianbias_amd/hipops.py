"""Host-side wrappers over the C-ABI: argument checking, output allocation (torch owns device memory),
and `torch.autograd.Function`s for the differentiable ops.  Every function here launches HIP kernels from
libposekernels.so on the current torch stream; none has a PyTorch fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, stream_ptr
from .configs.config import check_test_scales

F32, I32 = torch.float32, torch.int32


def _chk(t, dtype=F32, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.PoseKernelError(f"{name}: expected a CUDA(HIP) tensor; the hot path has no CPU implementation")
    if t.dtype != dtype:
        raise _lib.PoseKernelError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


# ------------------------------------------------------------------------------------------------ T1 / T2
_LUT_CACHE = {}


def _call_if(n, name, *args):
    """Launch unless the batch is empty: the reference's tensor code returns empty results for B = 0 (a frame without detections), and a
    zero-size grid is a launch error.  Nothing is computed on the host either way: the outputs are already the right (empty) shape."""
    if n > 0:
        call(name, *args)


def _patch_lut(sigma: float, device):
    """Host-built LUT of the reference's float32 patch (datasets/coco_dataset.py:227-233), indexed by d²."""
    key = (float(sigma), str(device))
    if key not in _LUT_CACHE:
        size = 2 * (sigma * 3) + 1
        ax = np.arange(0, size, 1, np.float32)
        c = size // 2
        g = np.exp(-((ax[None, :] - c) ** 2 + (ax[:, None] - c) ** 2) / (2 * sigma ** 2))   # same float32 expression
        n, ci = g.shape[0], int(c)
        far = max(ci, n - 1 - ci)
        lut = np.zeros(2 * far * far + 1, np.float32)
        for j in range(n):
            for i in range(n):
                lut[(i - ci) ** 2 + (j - ci) ** 2] = g[j, i]
        _LUT_CACHE[key] = (torch.from_numpy(lut).to(device), n, ci)
    return _LUT_CACHE[key]


def gaussian_target(keypoints, visible, input_size, heatmap_size, sigma):
    """(B,K,2),(B,K) -> target (B,K,Hh,Wh), weight (B,K,1). Sizes are (W,H) as in the reference config."""
    kp, vis = _chk(keypoints, name="keypoints"), _chk(visible, name="visible")
    B, K = vis.shape
    wh, hh = int(heatmap_size[0]), int(heatmap_size[1])
    lut, n, c = _patch_lut(float(sigma), kp.device)
    target = torch.empty(B, K, hh, wh, dtype=F32, device=kp.device)
    weight = torch.empty(B, K, 1, dtype=F32, device=kp.device)
    _call_if(B * K, "pk_gaussian_target", kp, vis, lut, lut.numel(), target, weight, B, K, hh, wh,
         float(input_size[0]) / float(heatmap_size[0]), float(input_size[1]) / float(heatmap_size[1]), float(sigma) * 3, n, c,
         stream_ptr())
    return target, weight


def dense_target(keypoints, visible, input_size_hw, heatmap_size_hw, sigma):
    kp, vis = _chk(keypoints, name="keypoints"), _chk(visible, name="visible")
    B, K = vis.shape
    hh, hw = int(heatmap_size_hw[0]), int(heatmap_size_hw[1])
    hm = torch.empty(B, K, hh, hw, dtype=F32, device=kp.device)
    w = torch.empty(B, K, dtype=F32, device=kp.device)
    _call_if(B * K, "pk_dense_target", kp, vis, hm, w, B, K, hh, hw, float(np.float32(hw / input_size_hw[1])),
         float(np.float32(hh / input_size_hw[0])), float(sigma), stream_ptr())
    return hm, w


# ------------------------------------------------------------------------------------------------ decoders
def argmax_decode(heatmaps, mode=0):
    """-> index (B,K) int32, maxval (B,K), coords (B,K,2). mode 0 plain / 1 quarter-shift / 2 Taylor."""
    hm = _chk(heatmaps, name="heatmaps")
    B, K, H, W = hm.shape
    idx = torch.empty(B, K, dtype=I32, device=hm.device)
    mv = torch.empty(B, K, dtype=F32, device=hm.device)
    co = torch.empty(B, K, 2, dtype=F32, device=hm.device)
    _call_if(B * K, "pk_argmax_decode", hm, idx, mv, co, B * K, H, W, int(mode), stream_ptr())
    return idx, mv, co


_TAPS_CACHE = {}


def unbiased_taps(kernel=11):
    """The `kernel` float32 taps of the unbiased decode's smoothing, cached per size: a Gaussian derived from the size alone by OpenCV's
    rule, sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8, g_i = exp(-(i - c)^2 / (2 sigma^2)) in float64, divided by its float64 sum, then rounded to
    float32.  (OpenCV's fixed tables for k <= 7 are deliberately not imitated: one formula for every size.)"""
    k = int(kernel)
    if k != kernel or k < 3 or k > 31 or k % 2 == 0:
        raise _lib.PoseKernelError(f"unbiased_decode: kernel {kernel!r} (an odd size from 3 to 31)")
    if k not in _TAPS_CACHE:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
        g = np.exp(-(np.arange(k, dtype=np.float64) - (k - 1) // 2) ** 2 / (2 * sigma ** 2))
        taps = (g / g.sum()).astype(np.float32)
        taps.setflags(write=False)
        _TAPS_CACHE[k] = taps
    return _TAPS_CACHE[k]


def unbiased_decode(heatmaps, kernel=11):
    """Unbiased (DARK) decode, pk_unbiased_decode: (B,K,H,W) -> index (B,K) int32, maxval (B,K), coords (B,K,2), refined (B,K) uint8 (1 where
    the Newton step on the log of the smoothed map was taken, 0 where coords are the integer argmax).  The taps ride in the launch: no
    host synchronisation, no host-to-device copy, no allocation but the outputs."""
    taps = unbiased_taps(kernel)
    hm = _chk(heatmaps, name="heatmaps")
    if hm.dim() != 4:
        raise _lib.PoseKernelError(f"unbiased_decode: heatmaps {tuple(hm.shape)} are not (B, K, H, W)")
    B, K, H, W = hm.shape
    idx = torch.empty(B, K, dtype=I32, device=hm.device)
    mv = torch.empty(B, K, dtype=F32, device=hm.device)
    co = torch.empty(B, K, 2, dtype=F32, device=hm.device)
    ref = torch.empty(B, K, dtype=torch.uint8, device=hm.device)
    _call_if(B * K, "pk_unbiased_decode", hm, taps.ctypes.data, taps.size, idx, mv, co, ref, B * K, H, W, stream_ptr())
    return idx, mv, co, ref


def softargmax_refine_decode(heatmaps, offsets, alpha_param, fusion_weight_param, radius=2):
    hm = _chk(heatmaps, name="heatmaps")
    B, K, H, W = hm.shape
    off = None if offsets is None else _chk(offsets, name="offsets")
    co = torch.empty(B, K, 2, dtype=F32, device=hm.device)
    sc = torch.empty(B, K, dtype=F32, device=hm.device)
    _call_if(B * K, "pk_softargmax_refine_decode", hm, off, _chk(alpha_param.reshape(1)), None if off is None else _chk(fusion_weight_param.reshape(1)),
         co, sc, B * K, H, W, int(radius), stream_ptr())
    return co, sc


def window_refine(heatmaps, coords, window=5):
    hm, c = _chk(heatmaps), _chk(coords)
    B, K, H, W = hm.shape
    out = torch.empty_like(c)
    _call_if(B * K, "pk_window_refine", hm, c, out, B * K, H, W, int(window), stream_ptr())
    return out


def fused_blend(hp, maxvals, regression, sx, sy, reg_scale):
    hp = _chk(hp)
    out = torch.empty_like(hp)
    _call_if(hp.shape[0] * hp.shape[1], "pk_fused_blend", hp, None if maxvals is None else _chk(maxvals), None if regression is None else _chk(regression), out,
         hp.shape[0] * hp.shape[1], float(sx), float(sy), float(reg_scale), stream_ptr())
    return out


def affine_coords(coords, center, scale, mul_x, mul_y, mask_maxvals=None, threshold=0.0):
    c = _chk(coords)
    B, K = c.shape[:2]
    out = torch.empty_like(c)
    _call_if(B * K, "pk_affine_coords", c, _chk(center), _chk(scale), out, B, K, float(mul_x), float(mul_y),
         None if mask_maxvals is None else _chk(mask_maxvals), float(threshold), stream_ptr())
    return out


def pose_records(keypoints, scores):
    """(B,K,2), (B,K) -> records (B,K,3) = [x, y, score], instance score (B,) = mean of the positive scores (COCOEvaluator.update)."""
    kp, sc = _chk(keypoints, name="keypoints"), _chk(scores, name="scores")
    B, K = sc.shape
    rec = torch.empty(B, K, 3, dtype=F32, device=kp.device)
    inst = torch.empty(B, dtype=F32, device=kp.device)
    _call_if(B * K, "pk_pose_records", kp, sc, rec, inst, B, K, stream_ptr())
    return rec, inst


F64, I64 = torch.float64, torch.int64


def coco_kpt_oks(gt_kpt, gt_bbox, gt_area, gt_off, dt_kpt, dt_score, dt_off, vars_, cap_off, oks_off, max_dets):
    """computeOks of every image (pk_coco_kpt_oks).  gt_kpt (G,K,3), dt_kpt (N,K,3) fp64; *_off int32 CSR offsets over the images, oks_off
    int64; vars_ = (2 sigma)^2.  -> cap_idx (n_cap,) int32 = detection of each capped slot (per image by descending score), oks (flat
    fp64, one D_i x G_i block per image at oks_off[i])."""
    gk, dk = _chk(gt_kpt, F64, "gt_kpt"), _chk(dt_kpt, F64, "dt_kpt")
    go, do, co, oo = _chk(gt_off, I32, "gt_off"), _chk(dt_off, I32, "dt_off"), _chk(cap_off, I32, "cap_off"), _chk(oks_off, I64, "oks_off")
    n_img, K = go.numel() - 1, dk.shape[1]
    n_cap, n_oks = int(co[-1]), int(oo[-1])
    cap_idx = torch.empty(max(n_cap, 1), dtype=I32, device=dk.device)
    oks = torch.empty(max(n_oks, 1), dtype=F64, device=dk.device)
    _call_if(n_img * n_cap, "pk_coco_kpt_oks", gk, _chk(gt_bbox, F64, "gt_bbox"), _chk(gt_area, F64, "gt_area"), go, dk,
             _chk(dt_score, F64, "dt_score"), do, _chk(vars_, F64, "vars"), co, oo, cap_idx, oks, n_img, K, int(max_dets), stream_ptr())
    return cap_idx[:n_cap], oks[:n_oks]


def coco_kpt_eval(oks, oks_off, gt_off, gt_area, gt_flags, cap_off, cap_idx, dt_score, dt_area, area_rng, iou_thrs, rec_thrs):
    """evaluateImg + accumulate (pk_coco_kpt_eval) over the blocks of `coco_kpt_oks`.  area_rng (A,2), iou_thrs (T,), rec_thrs (R,) fp64.
    -> dict: precision (T,R,A), recall (T,A), dt_match / dt_ignore (A,T,n_cap), npig (n_img,A), order (n_cap,)."""
    go, co = _chk(gt_off, I32, "gt_off"), _chk(cap_off, I32, "cap_off")
    ar, it, rt = _chk(area_rng, F64, "area_rng"), _chk(iou_thrs, F64, "iou_thrs"), _chk(rec_thrs, F64, "rec_thrs")
    dev = ar.device
    n_img, n_gt, n_cap = go.numel() - 1, int(go[-1]), cap_idx.numel()
    A, T, R = ar.shape[0], it.numel(), rt.numel()
    out = {"precision": torch.empty(T, R, A, dtype=F64, device=dev), "recall": torch.empty(T, A, dtype=F64, device=dev),
           "dt_match": torch.empty(A, T, n_cap, dtype=I32, device=dev), "dt_ignore": torch.empty(A, T, n_cap, dtype=torch.uint8, device=dev),
           "npig": torch.empty(n_img, A, dtype=I32, device=dev), "order": torch.empty(n_cap, dtype=I32, device=dev)}
    ws = torch.empty(max(int(_lib.lib.pk_coco_kpt_eval_ws_floats(n_gt, n_cap, A, T)), 1), dtype=F32, device=dev)
    _call_if(n_img * n_gt * n_cap, "pk_coco_kpt_eval", _chk(oks, F64, "oks") if oks.numel() else ws, _chk(oks_off, I64, "oks_off"), go,
             _chk(gt_area, F64, "gt_area"), _chk(gt_flags, I32, "gt_flags"), co, _chk(cap_idx, I32, "cap_idx"), _chk(dt_score, F64, "dt_score"),
             _chk(dt_area, F64, "dt_area"), ar, it, rt, out["dt_match"], out["dt_ignore"], out["npig"], out["order"], ws, out["precision"],
             out["recall"], n_img, n_gt, n_cap, A, T, R, stream_ptr())
    return out


OKS_NMS_MAX_POSES = _lib.CONSTANTS["PK_NMS_MAX_POSES"]      # poses per image pk_oks_nms holds in LDS
OKS_NMS_MAX_K = _lib.CONSTANTS["PK_NMS_MAX_K"]


def pose_rescore(kpt, box_score=None, in_vis_thr=0.2):
    """(N,K,3) fp64 rows [x, y, keypoint score] (+ (N,) fp64 box scores or None = 1) -> (N,) fp64: box score x mean of the keypoint scores
    above `in_vis_thr`, 0 without one (pk_pose_rescore)."""
    if kpt.dim() != 3 or kpt.shape[-1] != 3:
        raise ValueError(f"kpt: expected (N, K, 3), got {tuple(kpt.shape)}")
    N, K = int(kpt.shape[0]), int(kpt.shape[1])
    if not 1 <= K <= OKS_NMS_MAX_K:
        raise ValueError(f"kpt: {K} keypoints (1 to {OKS_NMS_MAX_K})")
    if box_score is not None and tuple(box_score.shape) != (N,):
        raise ValueError(f"box_score: expected {(N,)}, got {tuple(box_score.shape)}")
    kp = _chk(kpt, F64, "kpt")
    bs = None if box_score is None else _chk(box_score, F64, "box_score")
    out = torch.empty(N, dtype=F64, device=kp.device)
    _call_if(N, "pk_pose_rescore", kp, bs, out, N, K, float(in_vis_thr), stream_ptr())
    return out


def oks_nms(kpt, area, score, off, vars_, thr, in_vis_thr=0.2, soft=False, max_dets=20):
    """OKS-NMS of the poses of every image (pk_oks_nms, one workgroup per image).  kpt (N,K,3), area (N,), score (N,), vars_ (K,) = (2 sigma)^2:
    fp64 device tensors; off: the n_img + 1 int32 CSR offsets, a host array / CPU tensor (uploaded here) or a device tensor (copied back
    once: the per-image limit is checked on the host, before the launch).  -> keep (N,) uint8, n_keep (n_img,) int32, order (N,) int32 (per
    image: kept local indices in selection order, then -1), out_score (N,) fp64 (0 where not kept)."""
    if kpt.dim() != 3 or kpt.shape[-1] != 3:
        raise ValueError(f"kpt: expected (N, K, 3), got {tuple(kpt.shape)}")
    N, K = int(kpt.shape[0]), int(kpt.shape[1])
    if not 1 <= K <= OKS_NMS_MAX_K:
        raise ValueError(f"kpt: {K} keypoints (1 to {OKS_NMS_MAX_K})")
    for t, name, shape in ((area, "area", (N,)), (score, "score", (N,)), (vars_, "vars", (K,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected {shape}, got {tuple(t.shape)}")
    off_dev = off if isinstance(off, torch.Tensor) and off.is_cuda else None
    off_host = np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off)
    if off_host.ndim != 1 or off_host.size < 2 or off_host.dtype != np.int32:
        raise ValueError(f"off: expected n_img + 1 int32 offsets in one dimension, got {off_host.dtype} {off_host.shape}")
    counts = np.diff(off_host.astype(np.int64))
    if off_host[0] != 0 or off_host[-1] != N or (counts < 0).any():
        raise ValueError(f"off: offsets must ascend from 0 to N = {N}")
    if not math.isfinite(thr) or (soft and not (thr > 0 and int(max_dets) > 0)):
        raise ValueError(f"oks_nms: thr must be finite, and soft mode needs thr > 0 and max_dets > 0 (got thr {thr}, max_dets {max_dets})")
    if counts.max() > OKS_NMS_MAX_POSES:
        i = int(counts.argmax())
        raise _lib.PoseKernelError(f"pk_oks_nms failed (code -2, PK_ERR_UNSUPPORTED): image {i} holds {int(counts[i])} poses; the kernel is "
                                   f"built for at most {OKS_NMS_MAX_POSES} per image")
    kp, ar, sc, va = _chk(kpt, F64, "kpt"), _chk(area, F64, "area"), _chk(score, F64, "score"), _chk(vars_, F64, "vars")
    dev, n_img = kp.device, int(off_host.size) - 1
    od = _chk(off_dev, I32, "off") if off_dev is not None else torch.from_numpy(np.ascontiguousarray(off_host)).to(dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    n_keep = torch.zeros(n_img, dtype=I32, device=dev)
    order = torch.empty(N, dtype=I32, device=dev)
    out_score = torch.empty(N, dtype=F64, device=dev)
    _call_if(N, "pk_oks_nms", kp, ar, sc, od, va, keep, n_keep, order, out_score, n_img, K, float(thr), float(in_vis_thr), int(bool(soft)),
             int(max_dets), stream_ptr())
    return keep, n_keep, order, out_score


def flip_merge(hm, hm_from_flipped, partner):
    a, b = _chk(hm), _chk(hm_from_flipped)
    B, K, H, W = a.shape
    out = torch.empty_like(a)
    _call_if(B * K, "pk_flip_merge", a, b, _chk(partner, I32), out, B, K, H, W, stream_ptr())
    return out


def multiscale_merge(stack, scales, B, partner=None, flip=False):
    """Multi-scale (flip) test merge, pk_multiscale_merge: stack (S*F*B, K, H, W) pass-major (pass s*F + f; f = 1 the mirrored crop's
    forward, F = 2 with `flip`), `scales` in pass order -> (B, K, H, W) in the frame of the scale-1.0 crop."""
    try:
        sc = check_test_scales(scales)
    except ValueError as e:
        raise _lib.PoseKernelError(f"multiscale_merge: {e}") from None
    S, F, B = len(sc), 2 if flip else 1, int(B)
    if not isinstance(stack, torch.Tensor) or stack.dim() != 4 or B < 0 or stack.shape[0] != S * F * B:
        raise _lib.PoseKernelError(f"multiscale_merge: stack {tuple(getattr(stack, 'shape', ()))} is not (S*F*B = {S}*{F}*{B}, K, H, W)")
    st = _chk(stack, name="stack")
    if flip and partner is None:
        raise _lib.PoseKernelError("multiscale_merge: flip needs the partner table")
    K, H, W = st.shape[1:]
    if flip and _chk(partner, I32, "partner").numel() != K:
        raise _lib.PoseKernelError(f"multiscale_merge: partner has {partner.numel()} entries for K = {K}")
    inv = np.array([1.0 / s for s in sc], np.float64).astype(np.float32)      # float32(1 / float64(scale)); copied into the launch
    out = torch.empty(B, K, H, W, dtype=F32, device=st.device)
    _call_if(B * K * H * W, "pk_multiscale_merge", st, _chk(partner, I32, "partner") if flip else None, inv.ctypes.data, out, S, F, B, K, H, W,
             stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ losses
def loss_ws_floats(B, K):
    return B * K * 24 + B * 16 * 4 + 16


class _FusionLoss(torch.autograd.Function):
    """L1/L2 forward + hand-derived backward (fusion_head.py:745-806). Returns the 7 loss values as one tensor."""

    @staticmethod
    def forward(ctx, hm, off, var, target, weight, gt, in_w, in_h, sigma_t, lambdas, use_target_weight=True):
        hm, off, var = _chk(hm, name="heatmaps"), _chk(off, name="offsets"), _chk(var, name="variances")
        target, weight, gt = _chk(target), _chk(weight), _chk(gt)
        B, K, H, W = hm.shape
        if off.shape != (B, K, 2, H, W) or var.shape != hm.shape or target.shape != hm.shape or weight.numel() != B * K or gt.shape != (B, K, 2):
            raise _lib.PoseKernelError("fusion loss: inconsistent shapes")
        if lambdas.numel() == 6:           # term weights only: default overlap threshold (fusion_head.py:404)
            lambdas = torch.cat([lambdas.float(), lambdas.new_full((1,), 0.5, dtype=F32)])
        lambdas = _chk(lambdas.float(), name="lambdas")
        ws = torch.empty(loss_ws_floats(B, K), dtype=F32, device=hm.device)
        losses = torch.empty(7, dtype=F32, device=hm.device)
        call("pk_fusion_loss_fwd", hm, off, var, target, weight, gt, ws, losses, B, K, H, W, float(in_w), float(in_h), float(sigma_t),
             lambdas, 1 if use_target_weight else 0, stream_ptr())
        ctx.save_for_backward(hm, off, var, target, weight, ws, lambdas)
        ctx.sigma_t = float(sigma_t)
        return losses

    @staticmethod
    def backward(ctx, g):
        hm, off, var, target, weight, ws, lambdas = ctx.saved_tensors
        B, K, H, W = hm.shape
        # d(sum_i g_i * loss_i): entries 0..5 are the weighted terms and entry 6 their sum, so the per-term
        # multipliers are lambdas*(g[:6]+g[6]); the kernel takes them as "lambdas" with grad_total = 1.
        # (the kernel applies them: five tiny ATen launches at the very start of backward otherwise)
        dhm, doff, dvar = torch.empty_like(hm), torch.empty_like(off), torch.empty_like(var)
        call("pk_fusion_terms_bwd", hm, target, ws, None, None, _chk(g.float()), dhm, doff, dvar, None, B, K, H, W, ctx.sigma_t, lambdas,
             stream_ptr())
        return dhm, doff, dvar, None, None, None, None, None, None, None, None


def fusion_loss(hm, off, var, target, weight, gt, input_size, sigma_t, lambdas_dev, use_target_weight=True):
    return _FusionLoss.apply(hm, off, var, target, weight, gt, float(input_size[0]), float(input_size[1]), sigma_t, lambdas_dev,
                             bool(use_target_weight))


class _FusionTerms(torch.autograd.Function):
    """The seven loss values of pk_fusion_terms_fwd with the coordinates HANDED IN (None = the maps' own soft-argmax) plus the per-map
    sigma of compute_heatmap_variance; gradients for heatmaps, offsets, variances and the coordinates (fusion_head.py:405-575,637-743)."""

    @staticmethod
    def forward(ctx, hm, off, var, coords, target, weight, gt, in_w, in_h, sigma_t, lambdas, use_target_weight):
        hm, off, var = _chk(hm, name="heatmaps"), _chk(off, name="offsets"), _chk(var, name="variances")
        target, weight, gt = _chk(target), _chk(weight), _chk(gt)
        co = None if coords is None else _chk(coords, name="coords")
        B, K, H, W = hm.shape
        if off.shape != (B, K, 2, H, W) or var.shape != hm.shape or target.shape != hm.shape or weight.numel() != B * K or gt.shape != (B, K, 2) \
                or (co is not None and co.shape != (B, K, 2)):
            raise _lib.PoseKernelError("fusion terms: inconsistent shapes")
        lambdas = _chk(lambdas.float(), name="lambdas")
        ws = torch.empty(loss_ws_floats(B, K), dtype=F32, device=hm.device)
        losses = torch.empty(7, dtype=F32, device=hm.device)
        sigma = torch.empty(B, K, dtype=F32, device=hm.device)
        call("pk_fusion_terms_fwd", hm, off, var, target, weight, gt, co, ws, losses, sigma, B, K, H, W, float(in_w), float(in_h), float(sigma_t),
             lambdas, 1 if use_target_weight else 0, stream_ptr())
        ctx.save_for_backward(hm, target, ws, lambdas)
        ctx.meta = (float(sigma_t), co is not None, tuple(off.shape))
        return losses, sigma

    @staticmethod
    def backward(ctx, g, gsig):
        hm, target, ws, lambdas = ctx.saved_tensors
        sigma_t, ext, off_shape = ctx.meta
        B, K, H, W = hm.shape
        dhm, dvar = torch.empty_like(hm), torch.empty_like(hm)
        doff = torch.empty(off_shape, dtype=F32, device=hm.device)
        dco = torch.empty(B, K, 2, dtype=F32, device=hm.device) if ext else None
        call("pk_fusion_terms_bwd", hm, target, ws, None, None if gsig is None else _chk(gsig.float()), _chk(g.float()), dhm, doff, dvar, dco,
             B, K, H, W, sigma_t, lambdas, stream_ptr())
        return dhm, doff, dvar, dco, None, None, None, None, None, None, None, None


def fusion_terms(lambdas7, hm=None, off=None, var=None, coords=None, target=None, weight=None, gt=None, input_size=(1.0, 1.0),
                 sigma_t=2.0, use_target_weight=True, shape=None):
    """Per-term access to the fused loss kernels for the reference's public loss methods: inputs a method does not take are replaced by
    neutral device tensors (zero maps; variances == sigma_t, whose term is then exactly 0) and masked out by a zero lambda.
    -> (losses (7,), sigma (B,K))."""
    ref = hm if hm is not None else (off if off is not None else coords)
    dev = ref.device
    B, K, H, W = shape if shape is not None else hm.shape
    z = None

    def zeros():
        nonlocal z
        if z is None:
            z = torch.zeros(B, K, H, W, dtype=F32, device=dev)
        return z

    hm = zeros() if hm is None else hm.float()
    off = torch.zeros(B, K, 2, H, W, dtype=F32, device=dev) if off is None else off.float().reshape(B, K, 2, H, W)
    var = torch.full((B, K, H, W), float(sigma_t), dtype=F32, device=dev) if var is None else var.float()
    target = zeros() if target is None else target.float()
    weight = torch.ones(B, K, 1, dtype=F32, device=dev) if weight is None else weight.float()
    gt = torch.zeros(B, K, 2, dtype=F32, device=dev) if gt is None else gt.float()
    lam = torch.as_tensor(lambdas7, dtype=F32, device=dev) if not torch.is_tensor(lambdas7) else lambdas7
    return _FusionTerms.apply(hm, off, var, None if coords is None else coords.float(), target, weight, gt, float(input_size[0]),
                              float(input_size[1]), float(sigma_t), lam, bool(use_target_weight))


class _SoftArgmax(torch.autograd.Function):
    """SoftArgmax2D.forward with gradients (fusion_head.py:24-71): coords through the softmax, scores to the first maximum."""

    @staticmethod
    def forward(ctx, hm):
        hm = _chk(hm, name="heatmaps")
        one = torch.full((1,), 40.0, device=hm.device)          # sigmoid(40) == 1: pure global soft-argmax
        co, sc = softargmax_refine_decode(hm, None, one, None, radius=0)
        ctx.save_for_backward(hm, co, sc)
        return co, sc

    @staticmethod
    def backward(ctx, gco, gsc):
        hm, co, sc = ctx.saved_tensors
        B, K, H, W = hm.shape
        dhm = torch.empty_like(hm)
        call("pk_softargmax_bwd", hm, co, sc, None if gco is None else _chk(gco.float()), None if gsc is None else _chk(gsc.float()), dhm,
             B * K, H, W, stream_ptr())
        return dhm


def softargmax(hm):
    return _SoftArgmax.apply(hm)


def local_gaussian_refine(heatmaps, coords, radius=2):
    hm, c = _chk(heatmaps, name="heatmaps"), _chk(coords, name="coords")
    B, K, H, W = hm.shape
    out = torch.empty_like(c)
    call("pk_local_gaussian_refine", hm, c, out, B * K, H, W, int(radius), stream_ptr())
    return out


class _RowsByMap(torch.autograd.Function):
    """Rows moved through an int32 row map (window_partition = gather, window_reverse = scatter); the backward is the opposite move."""

    @staticmethod
    def forward(ctx, x2d, rowmap, n_out, scatter):
        x2d = x2d.contiguous()
        if not x2d.is_cuda or (x2d.shape[1] * x2d.element_size()) % 4:
            raise _lib.PoseKernelError("rows_by_map: CUDA(HIP) tensor with rows of whole dwords expected")
        out = (torch.zeros if scatter else torch.empty)((n_out, x2d.shape[1]), dtype=x2d.dtype, device=x2d.device)
        call("pk_rows_by_map", x2d, out, rowmap, rowmap.numel(), x2d.shape[1] * x2d.element_size(), 1 if scatter else 0, stream_ptr())
        ctx.save_for_backward(rowmap)
        ctx.meta = (x2d.shape[0], scatter)
        return out

    @staticmethod
    def backward(ctx, g):
        (rowmap,) = ctx.saved_tensors
        n_in, scatter = ctx.meta
        return _RowsByMap.apply(g, rowmap, n_in, not scatter), None, None, None


def rows_by_map(x2d, rowmap, n_out, scatter):
    return _RowsByMap.apply(x2d, rowmap, n_out, scatter)


class _DropPath(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, keep):
        x = _chk(x, name="x")
        out = torch.empty_like(x)
        call("pk_drop_path_f32", x, mask, out, x.shape[0], x.numel() // x.shape[0], float(keep), stream_ptr())
        ctx.save_for_backward(mask)
        ctx.keep = keep
        return out

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return _DropPath.apply(g.float().contiguous(), mask, ctx.keep), None, None


def drop_path(x, mask, keep):
    return _DropPath.apply(x, mask, keep)


class _PixelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, kind):
        pred, target = _chk(pred), _chk(target)
        B, K = pred.shape[:2]
        HW = pred.numel() // (B * K)
        w = None if weight is None else _chk(weight)
        partial = torch.empty(1024, dtype=F32, device=pred.device)
        loss = torch.empty(1, dtype=F32, device=pred.device)
        call("pk_pixel_loss_fwd", pred, target, w, partial, loss, B, K, HW, kind, stream_ptr())
        ctx.save_for_backward(pred, target, w if w is not None else pred.new_empty(0))
        ctx.kind, ctx.has_w = kind, w is not None
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, target, w = ctx.saved_tensors
        B, K = pred.shape[:2]
        dp = torch.empty_like(pred)
        call("pk_pixel_loss_bwd", pred, target, w if ctx.has_w else None, _chk(g.reshape(1).float()), dp, B, K, pred.numel() // (B * K), ctx.kind,
             stream_ptr())
        return dp, None, None, None


def pixel_loss(pred, target, weight, kind):
    return _PixelLoss.apply(pred, target, weight, int(kind))


class _OhkmLoss(torch.autograd.Function):
    """Online hard keypoint mining (pk_ohkm_loss_fwd / _bwd): the selection happens on the device, the mask it leaves is what backward reads."""

    @staticmethod
    def forward(ctx, pred, target, weight, topk, scale, counts):
        pred, target = _chk(pred, name="pred"), _chk(target, name="target")
        if pred.dim() < 3 or target.shape != pred.shape:
            raise _lib.PoseKernelError(f"ohkm_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be the same (B,K,...) maps")
        B, K = pred.shape[:2]
        HW = pred.numel() // max(B * K, 1)
        w = None if weight is None else _chk(weight, name="weight")
        if w is not None and w.numel() != B * K:
            raise _lib.PoseKernelError(f"ohkm_loss: weight has {w.numel()} elements, expected B*K = {B * K}")
        if counts is not None:
            _chk(counts, torch.int64, "counts")
            if counts.shape != (K,) or not counts.is_contiguous():
                raise _lib.PoseKernelError(f"ohkm_loss: counts must be a contiguous int64 ({K},) tensor, got {tuple(counts.shape)}")
        per_map = torch.empty(B, K, dtype=F32, device=pred.device)
        mask = torch.empty(B, K, dtype=torch.uint8, device=pred.device)
        loss = torch.empty(1, dtype=F32, device=pred.device)
        call("pk_ohkm_loss_fwd", pred, target, w, per_map, mask, loss, counts, B, K, HW, int(topk), float(scale), stream_ptr())
        ctx.save_for_backward(pred, target, w if w is not None else pred.new_empty(0), mask)
        ctx.topk, ctx.scale, ctx.has_w = int(topk), float(scale), w is not None
        ctx.mark_non_differentiable(per_map, mask)
        return loss.reshape(()), per_map, mask

    @staticmethod
    def backward(ctx, g, _g_per_map, _g_mask):
        pred, target, w, mask = ctx.saved_tensors
        B, K = pred.shape[:2]
        dp = torch.empty_like(pred)
        call("pk_ohkm_loss_bwd", pred, target, w if ctx.has_w else None, mask, _chk(g.reshape(1).float()), dp, B, K, pred.numel() // (B * K),
             ctx.topk, ctx.scale, stream_ptr())
        return dp, None, None, None, None, None


def ohkm_loss(pred, target, weight, topk, scale=1.0, counts=None, return_selection=False):
    """scale / (B topk) * sum over every sample's `topk` hardest maps of mean((w (pred - target))^2), as a scalar.  `counts`: an int64 (K,)
    device tensor that gains the number of samples each joint was selected in.  `return_selection`: also the per-map errors (B,K) and the
    uint8 selection mask (B,K), neither differentiable."""
    loss, per_map, mask = _OhkmLoss.apply(pred, target, weight, topk, scale, counts)
    return (loss, per_map, mask) if return_selection else loss


class _SpatialStats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm):
        hm = _chk(hm)
        B, K, H, W = hm.shape
        mean = torch.empty(B, K, 2, dtype=F32, device=hm.device)
        var = torch.empty(B, K, 2, dtype=F32, device=hm.device)
        call("pk_spatial_stats", hm, mean, var, B * K, H, W, stream_ptr())
        ctx.save_for_backward(hm, mean, var)
        return mean, var

    @staticmethod
    def backward(ctx, gmean, gvar):
        hm, mean, var = ctx.saved_tensors
        B, K, H, W = hm.shape
        gmean = torch.zeros_like(mean) if gmean is None else gmean.contiguous().float()
        gvar = torch.zeros_like(var) if gvar is None else gvar.contiguous().float()
        dhm = torch.empty_like(hm)
        call("pk_spatial_stats_bwd", hm, mean, var, gmean, gvar, dhm, B * K, H, W, stream_ptr())
        return dhm


def spatial_stats(hm):
    """centre of mass and per-axis variance of hm/(sum+1e-8): (B,K,2), (B,K,2); differentiable w.r.t. hm."""
    return _SpatialStats.apply(hm)


def temporal_smooth(coords, kernel):
    coords = _chk(coords)
    T, K, _ = coords.shape
    w = torch.as_tensor(kernel, dtype=torch.float64).to(coords.device)
    out = torch.empty_like(coords)
    call("pk_temporal_smooth", coords, out, w, T, K * 2, int(w.numel()), stream_ptr())
    return out


def nms_pose(preds, maxvals, distance_threshold=5.0):
    preds, maxvals = _chk(preds), _chk(maxvals.reshape(preds.shape[0], preds.shape[1]))
    B, K, _ = preds.shape
    out = torch.empty_like(preds)
    keep = torch.empty(B, K, dtype=torch.uint8, device=preds.device)
    _call_if(B * K, "pk_nms_pose", preds, maxvals, out, keep, B, K, float(distance_threshold), stream_ptr())
    return out, keep.bool().view(B, K, 1)


# ------------------------------------------------------------------------------------------------ movement analysis and PCK
PCK_MAX_THRESHOLDS = _lib.CONSTANTS["PK_PCK_MAX_THR"]
HIST_MAX_BINS = _lib.CONSTANTS["PK_HIST_MAX_BINS"]


def pck_buffers(num_keypoints, n_thr, device):
    """Zeroed accumulators of `pck_accumulate`: correct (n_thr, K) int64, valid (K,) int64, err_sum (K,) float64."""
    return (torch.zeros(n_thr, num_keypoints, dtype=I64, device=device), torch.zeros(num_keypoints, dtype=I64, device=device),
            torch.zeros(num_keypoints, dtype=F64, device=device))


def pck_accumulate(pred, gt, visible, normalizer, thresholds, correct, valid, err_sum):
    """One batch into the PCK accumulators, in place (pk_pck; no synchronisation).  pred, gt (N,K,2); visible (N,K); normalizer (N,);
    thresholds (n_thr,) float32 device tensor; correct (n_thr,K) / valid (K,) int64 and err_sum (K,) float64 from `pck_buffers`.
    Shapes are checked first (ValueError), then every tensor's device and type (PoseKernelError); nothing is launched before both."""
    if pred.dim() != 3 or pred.shape[-1] != 2:
        raise ValueError(f"pred: expected (N, K, 2), got {tuple(pred.shape)}")
    N, K = int(pred.shape[0]), int(pred.shape[1])
    n_thr = int(thresholds.numel())
    if gt.shape != pred.shape:
        raise ValueError(f"gt: expected {tuple(pred.shape)} like pred, got {tuple(gt.shape)}")
    if tuple(visible.shape) != (N, K):
        raise ValueError(f"visible: expected {(N, K)}, got {tuple(visible.shape)}")
    if tuple(normalizer.shape) != (N,):
        raise ValueError(f"normalizer: expected {(N,)}, got {tuple(normalizer.shape)}")
    if thresholds.dim() != 1 or not 1 <= n_thr <= PCK_MAX_THRESHOLDS:
        raise ValueError(f"thresholds: expected 1 to {PCK_MAX_THRESHOLDS} values in one dimension, got {tuple(thresholds.shape)}")
    if tuple(correct.shape) != (n_thr, K) or tuple(valid.shape) != (K,) or tuple(err_sum.shape) != (K,):
        raise ValueError(f"accumulators: expected {(n_thr, K)}, {(K,)}, {(K,)}, got {tuple(correct.shape)}, {tuple(valid.shape)}, "
                         f"{tuple(err_sum.shape)}")
    for t, name in ((correct, "correct"), (valid, "valid"), (err_sum, "err_sum")):
        if not t.is_contiguous():
            raise ValueError(f"{name}: the accumulators are updated in place and must be contiguous")
    pred, gt = _chk(pred, name="pred"), _chk(gt, name="gt")
    vis, norm, thr = _chk(visible, name="visible"), _chk(normalizer, name="normalizer"), _chk(thresholds, name="thresholds")
    correct, valid, err_sum = _chk(correct, I64, "correct"), _chk(valid, I64, "valid"), _chk(err_sum, F64, "err_sum")
    _call_if(N * K, "pk_pck", pred, gt, vis, norm, thr, correct, valid, err_sum, N, K, n_thr, stream_ptr())


def _sequences(coords, conf):
    """coords (S,T,K,2) and conf (S,T,K) or None: shapes (ValueError), then device and type -> coords, conf, S, T, K."""
    if coords.dim() != 4 or coords.shape[-1] != 2:
        raise ValueError(f"coords: expected (S, T, K, 2), got {tuple(coords.shape)}")
    if conf is not None and conf.shape != coords.shape[:3]:
        raise ValueError(f"conf: expected {tuple(coords.shape[:3])}, got {tuple(conf.shape)}")
    coords = _chk(coords, name="coords")
    conf = None if conf is None else _chk(conf, name="conf")
    return (coords, conf) + tuple(int(v) for v in coords.shape[:3])


def motion_stats(coords, conf=None, min_conf=0.3):
    """(S,T,K,2) image-pixel trajectories (+ (S,T,K) confidences) -> (S,K,11) float64 per-joint statistics (pk_motion_stats: n_valid,
    min_x, max_x, min_y, max_y, amplitude, path length, n_steps, largest step, second-difference sum, n_triples)."""
    coords, conf, S, T, K = _sequences(coords, conf)
    stats = torch.zeros(S, K, 11, dtype=F64, device=coords.device)
    _call_if(S * T * K, "pk_motion_stats", coords, conf, stats, S, T, K, float(min_conf), stream_ptr())
    return stats


def position_histogram(coords, edges_x, edges_y, conf=None, min_conf=0.3):
    """(S,T,K,2) trajectories -> (S,K,nby,nbx) int32 counts of the valid frames per bin of the ascending float64 edges (host arrays or
    device tensors of nbx + 1 / nby + 1 values), np.histogram2d's rule (pk_position_histogram)."""
    ex, ey = (e.to(F64) if isinstance(e, torch.Tensor) else torch.from_numpy(np.array(e, dtype=np.float64)) for e in (edges_x, edges_y))
    if ex.dim() != 1 or ey.dim() != 1 or ex.numel() < 2 or ey.numel() < 2:
        raise ValueError(f"edges: expected one-dimensional arrays of at least 2 values, got {tuple(ex.shape)} and {tuple(ey.shape)}")
    coords, conf, S, T, K = _sequences(coords, conf)
    ex, ey = _chk(ex.to(coords.device), F64, "edges_x"), _chk(ey.to(coords.device), F64, "edges_y")
    nbx, nby = int(ex.numel()) - 1, int(ey.numel()) - 1
    counts = torch.zeros(S, K, nby, nbx, dtype=I32, device=coords.device)
    _call_if(S * T * K, "pk_position_histogram", coords, conf, ex, ey, counts, S, T, K, nbx, nby, float(min_conf), stream_ptr())
    return counts


SPECTRUM_MAX_BINS = _lib.CONSTANTS["PK_SPEC_MAX_BINS"]
SPECTRUM_MAX_NFFT = _lib.CONSTANTS["PK_SPEC_MAX_NFFT"]


def motion_spectrum(coords, conf=None, min_conf=0.3, n_fft=None, j0=1, n_bins=None, window=1):
    """(S,T,K,2) image-pixel trajectories (+ (S,T,K) confidences) -> power (S,K,F) and summary (S,K,6), float64 (pk_motion_spectrum).
    Bin j is the frequency (j0 + j) / n_fft cycles per frame (n_fft: T when None; larger zero-pads; n_bins: up to n_fft // 2 when None);
    window 0 rectangular, 1 periodic Hann.  A linear oscillation of amplitude A px at a bin frequency has power A^2.  Summary columns:
    valid frames, window sum, band power, peak bin (-1 without power), peak power, centroid in bins."""
    coords, conf, S, T, K = _sequences(coords, conf)
    N = T if n_fft is None else int(n_fft)
    j0 = int(j0)
    F = N // 2 - j0 + 1 if n_bins is None else int(n_bins)
    if not 2 <= N <= SPECTRUM_MAX_NFFT:
        raise ValueError(f"n_fft: expected 2 to {SPECTRUM_MAX_NFFT}, got {N}")
    if j0 < 1 or F < 1 or j0 + F - 1 > N // 2:
        raise ValueError(f"bins {j0} to {j0 + F - 1}: expected a non-empty range inside 1 to n_fft // 2 = {N // 2}")
    if F > SPECTRUM_MAX_BINS:
        raise ValueError(f"n_bins: {F} bins in one call (at most {SPECTRUM_MAX_BINS}); take the band in parts")
    if window not in (0, 1):
        raise ValueError(f"window: expected 0 (rectangular) or 1 (Hann), got {window!r}")
    power = torch.zeros(S, K, F, dtype=F64, device=coords.device)
    summary = torch.zeros(S, K, 6, dtype=F64, device=coords.device)
    if S * T * K > 0:
        call("pk_motion_spectrum", coords, conf, power, summary, S, T, K, float(min_conf), N, j0, F, int(window), stream_ptr())
    else:
        summary[..., 3] = -1.0                                    # no frame: no power, no peak
    return power, summary


# ------------------------------------------------------------------------------------------------ limb kinematics
KIN_MAX_ANGLES = _lib.CONSTANTS["PK_KIN_MAX_ANGLES"]
KIN_MAX_LAG = _lib.CONSTANTS["PK_KIN_MAX_LAG"]
KIN_MAX_M = _lib.CONSTANTS["PK_KIN_MAX_M"]
KIN_MAX_T = _lib.CONSTANTS["PK_KIN_MAX_T"]
KIN_STATS_COLS = _lib.CONSTANTS["PK_KIN_STATS_COLS"]


def _index_table(table, width, limit, name, what, distinct_neighbours=False):
    """A host list / array (or tensor) of index rows -> (n, width) int32 numpy array, every entry in [0, limit): ValueError naming the row."""
    rows = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table)
    if rows.ndim != 2 or rows.shape[1] != width or rows.shape[0] < 1 or rows.dtype.kind not in "iu":
        raise ValueError(f"{name}: expected at least one row of {width} integer {what}, got {rows.dtype} {tuple(rows.shape)}")
    rows = rows.astype(np.int64)
    for i, row in enumerate(rows):
        if (row < 0).any() or (row >= limit).any():
            raise ValueError(f"{name}[{i}] = {tuple(int(v) for v in row)}: {what} lie in 0 to {limit - 1}")
        if distinct_neighbours and (row[0] == row[1] or row[1] == row[2]):
            raise ValueError(f"{name}[{i}] = {tuple(int(v) for v in row)}: the middle joint must differ from both ends")
    return np.ascontiguousarray(rows, np.int32)


def _series(series, name="series"):
    """series (S,T,Q) float64: shape (ValueError) -> S, T, Q."""
    if series.dim() != 3:
        raise ValueError(f"{name}: expected (S, T, Q), got {tuple(series.shape)}")
    return tuple(int(v) for v in series.shape)


def joint_angles(coords, conf, min_conf, triples):
    """(S,T,K,2) image-pixel trajectories (+ (S,T,K) confidences or None) and `triples`, a host list of joints (a, b, c) -> (S,T,A) float64:
    the unsigned interior angle at b in radians, NaN where one of the three joints is invalid or coincides with b (pk_joint_angles)."""
    if coords.dim() != 4 or coords.shape[-1] != 2:
        raise ValueError(f"coords: expected (S, T, K, 2), got {tuple(coords.shape)}")
    tri = _index_table(triples, 3, int(coords.shape[2]), "triples", "joints", distinct_neighbours=True) if coords.shape[2] > 0 else None
    if tri is None or not 1 <= tri.shape[0] <= KIN_MAX_ANGLES:
        raise ValueError(f"triples: expected 1 to {KIN_MAX_ANGLES} angles over at least one joint")
    coords, conf, S, T, K = _sequences(coords, conf)
    A = int(tri.shape[0])
    angles = torch.full((S, T, A), float("nan"), dtype=F64, device=coords.device)
    if S * T > 0:
        call("pk_joint_angles", coords, conf, torch.from_numpy(tri).to(coords.device), angles, S, T, K, A, float(min_conf), stream_ptr())
    return angles


def joint_speeds(coords, conf=None, min_conf=0.3):
    """(S,T,K,2) trajectories -> (S,T,K) float64: |p[t+1] - p[t]| in pixels per frame where both frames are valid, else NaN (pk_joint_speeds)."""
    coords, conf, S, T, K = _sequences(coords, conf)
    speeds = torch.full((S, T, K), float("nan"), dtype=F64, device=coords.device)
    _call_if(S * T * K, "pk_joint_speeds", coords, conf, speeds, S, T, K, float(min_conf), stream_ptr())
    return speeds


def series_stats(series):
    """(S,T,Q) float64 series (NaN = no value) -> (S,Q,8) float64 (pk_series_stats: n, min, max, mean, population sd, sum of |steps|, number
    of steps, largest step)."""
    S, T, Q = _series(series)
    series = _chk(series, F64, "series")
    stats = torch.zeros(S, Q, KIN_STATS_COLS, dtype=F64, device=series.device)
    _call_if(S * T * Q, "pk_series_stats", series, stats, S, T, Q, stream_ptr())
    return stats


def series_xcorr(series, pairs, max_lag, min_count=2):
    """(S,T,Q) float64 series and `pairs`, a host list of series (i, j) -> corr (S,P,2L+1) float64, count (S,P,2L+1) int32 and summary (S,P,4)
    float64 (pk_series_xcorr): Pearson's r of x_i[t] against x_j[t + l] over the co-valid frames of each lag l = -L .. L, and per pair r at
    lag 0, the lag of the largest r, that r and its pair count over the lags with at least `min_count` pairs."""
    S, T, Q = _series(series)
    L, min_count = int(max_lag), int(min_count)
    if not 0 <= L <= KIN_MAX_LAG:
        raise ValueError(f"max_lag: expected 0 to {KIN_MAX_LAG}, got {max_lag}")
    if min_count < 2:
        raise ValueError(f"min_count: expected at least 2 (one pair has no correlation), got {min_count}")
    if Q < 1:
        raise ValueError(f"series: expected at least one series, got {tuple(series.shape)}")
    pr = _index_table(pairs, 2, Q, "pairs", "series")
    series = _chk(series, F64, "series")
    P = int(pr.shape[0])
    corr = torch.zeros(S, P, 2 * L + 1, dtype=F64, device=series.device)
    count = torch.zeros(S, P, 2 * L + 1, dtype=I32, device=series.device)
    summary = torch.zeros(S, P, 4, dtype=F64, device=series.device)
    if S * T > 0:
        call("pk_series_xcorr", series, torch.from_numpy(pr).to(series.device), corr, count, summary, S, T, Q, P, L, min_count, stream_ptr())
    return corr, count, summary


def sample_entropy_tiles(T, m):
    """Partial-count rows per series of `sample_entropy_counts` (pk_sample_entropy_tiles)."""
    return int(_lib.lib.pk_sample_entropy_tiles(int(T), int(m)))


def sample_entropy_counts(series, tol, m=2, workspace=None):
    """(S,T,Q) float64 series and their absolute tolerances (S,Q) float64 -> (S,Q,3) int64: the number of valid templates of length m + 1, and
    the pairs of them that match within `tol` over m and over m + 1 elements, B and A of SampEn = -ln(A / B) (pk_sample_entropy).
    workspace: None, or an int64 tensor of at least S Q sample_entropy_tiles(T, m) rows of 2 to use instead of a fresh one."""
    S, T, Q = _series(series)
    if tuple(tol.shape) != (S, Q):
        raise ValueError(f"tol: expected {(S, Q)}, got {tuple(tol.shape)}")
    m = int(m)
    if not 1 <= m <= KIN_MAX_M:
        raise ValueError(f"m: expected 1 to {KIN_MAX_M}, got {m}")
    if T > KIN_MAX_T:
        raise ValueError(f"series: {T} frames exceed the {KIN_MAX_T} of one call; analyse it in windows")
    rows = S * Q * sample_entropy_tiles(T, m)
    if workspace is not None and workspace.numel() < 2 * max(rows, 1):
        raise ValueError(f"workspace: expected at least {2 * max(rows, 1)} int64, got {workspace.numel()}")
    series, tol = _chk(series, F64, "series"), _chk(tol, F64, "tol")
    workspace = torch.empty(max(rows, 1), 2, dtype=I64, device=series.device) if workspace is None else _chk(workspace, I64, "workspace")
    counts = torch.zeros(S, Q, 3, dtype=I64, device=series.device)
    _call_if(S * T * Q, "pk_sample_entropy", series, tol, workspace, counts, S, T, Q, m, stream_ptr())
    return counts


# ------------------------------------------------------------------------------------------------ localisation error analysis
ERR_MAX_BINS = _lib.CONSTANTS["PK_ERR_MAX_BINS"]
ERR_MAX_CONF_THRESHOLDS = _lib.CONSTANTS["PK_ERR_MAX_CONF_THR"]
ERR_MAX_QUANTILES = _lib.CONSTANTS["PK_ERR_MAX_QUANTILES"]
ERR_MAX_COLS = _lib.CONSTANTS["PK_ERR_MAX_COLS"]


def kpt_error_buffers(num_keypoints, n_bins, n_thr, device):
    """Zeroed counters of `kpt_error_accumulate`: calib_count, calib_hit (K, n_bins) int64 and pr_hist (K, 2, n_thr + 1) int64."""
    return (torch.zeros(num_keypoints, n_bins, dtype=I64, device=device), torch.zeros(num_keypoints, n_bins, dtype=I64, device=device),
            torch.zeros(num_keypoints, 2, n_thr + 1, dtype=I64, device=device))


def kpt_error_accumulate(pred, gt, visible, store, column, pixel_threshold, confidence=None, normalizer=None, bin_edges=None,
                         conf_thresholds=None, calib_count=None, calib_hit=None, pr_hist=None):
    """One batch into the error store and the counters, in place (pk_kpt_error; no synchronisation).  pred, gt (N,K,2); visible (N,K);
    store (K, capacity) float32, row-contiguous: columns column .. column + N - 1 of every row are written (NaN for a pair that does not
    count).  normalizer (N,) or None (errors in pixels).  confidence (N,K) or None; with one, bin_edges (n_bins + 1,) and conf_thresholds
    (T,) ascending float32 device tensors and the three int64 counters of `kpt_error_buffers` are needed and updated.
    Shapes are checked first (ValueError), then every tensor's device and type (PoseKernelError); nothing is launched before both."""
    if pred.dim() != 3 or pred.shape[-1] != 2:
        raise ValueError(f"pred: expected (N, K, 2), got {tuple(pred.shape)}")
    N, K, column = int(pred.shape[0]), int(pred.shape[1]), int(column)
    if gt.shape != pred.shape:
        raise ValueError(f"gt: expected {tuple(pred.shape)} like pred, got {tuple(gt.shape)}")
    if tuple(visible.shape) != (N, K):
        raise ValueError(f"visible: expected {(N, K)}, got {tuple(visible.shape)}")
    if normalizer is not None and tuple(normalizer.shape) != (N,):
        raise ValueError(f"normalizer: expected {(N,)}, got {tuple(normalizer.shape)}")
    if store.dim() != 2 or store.shape[0] != K or column < 0 or column + N > store.shape[1]:
        raise ValueError(f"store: expected ({K}, at least {column + N}) for {N} columns from column {column}, got {tuple(store.shape)}")
    if store.shape[1] > 0 and store.stride(1) != 1:
        raise ValueError("store: the error store is written in place and its rows must be contiguous")
    n_bins = n_thr = 0
    if confidence is not None:
        if tuple(confidence.shape) != (N, K):
            raise ValueError(f"confidence: expected {(N, K)}, got {tuple(confidence.shape)}")
        if bin_edges is None or conf_thresholds is None or calib_count is None or calib_hit is None or pr_hist is None:
            raise ValueError("confidence: needs bin_edges, conf_thresholds and the three counters of kpt_error_buffers")
        n_bins, n_thr = int(bin_edges.numel()) - 1, int(conf_thresholds.numel())
        if bin_edges.dim() != 1 or not 1 <= n_bins <= ERR_MAX_BINS:
            raise ValueError(f"bin_edges: expected the 2 to {ERR_MAX_BINS + 1} edges of 1 to {ERR_MAX_BINS} bins in one dimension, "
                             f"got {tuple(bin_edges.shape)}")
        if conf_thresholds.dim() != 1 or not 1 <= n_thr <= ERR_MAX_CONF_THRESHOLDS:
            raise ValueError(f"conf_thresholds: expected 1 to {ERR_MAX_CONF_THRESHOLDS} values in one dimension, "
                             f"got {tuple(conf_thresholds.shape)}")
        if tuple(calib_count.shape) != (K, n_bins) or tuple(calib_hit.shape) != (K, n_bins) or tuple(pr_hist.shape) != (K, 2, n_thr + 1):
            raise ValueError(f"counters: expected {(K, n_bins)}, {(K, n_bins)}, {(K, 2, n_thr + 1)}, got {tuple(calib_count.shape)}, "
                             f"{tuple(calib_hit.shape)}, {tuple(pr_hist.shape)}")
        for t, name in ((calib_count, "calib_count"), (calib_hit, "calib_hit"), (pr_hist, "pr_hist")):
            if not t.is_contiguous():
                raise ValueError(f"{name}: the counters are updated in place and must be contiguous")
    pred, gt, vis = _chk(pred, name="pred"), _chk(gt, name="gt"), _chk(visible, name="visible")
    norm = None if normalizer is None else _chk(normalizer, name="normalizer")
    if not (isinstance(store, torch.Tensor) and store.is_cuda and store.dtype == F32):
        raise _lib.PoseKernelError("store: expected a float32 CUDA(HIP) tensor; the hot path has no CPU implementation")
    conf = edges = thr = None
    if confidence is not None:
        conf, edges, thr = _chk(confidence, name="confidence"), _chk(bin_edges, name="bin_edges"), _chk(conf_thresholds, name="conf_thresholds")
        calib_count, calib_hit, pr_hist = _chk(calib_count, I64, "calib_count"), _chk(calib_hit, I64, "calib_hit"), _chk(pr_hist, I64, "pr_hist")
    else:
        calib_count = calib_hit = pr_hist = None
    if N * K > 0:
        first = store.data_ptr() + 4 * column                     # the first free column of row 0; row k starts ld floats further
        call("pk_kpt_error", pred, gt, vis, conf, norm, float(pixel_threshold), edges, n_bins, thr, n_thr, first, int(store.stride(0)),
             calib_count, calib_hit, pr_hist, N, K, stream_ptr())


def kpt_error_quantiles(store, n_cols, q):
    """Exact order statistics of the first n_cols columns of every row of the (K, capacity) float32 error store (pk_kpt_error_quantiles;
    no synchronisation).  q (Q,) float64 device tensor, each in [0, 1].  -> order (K,Q,2) float32: the values v[lo], v[hi] around position
    q (n - 1) of the row's n non-NaN values in ascending order; summary (K,4) float64: n, sum, min, max.  All zero for a row without a value
    and for n_cols = 0 (nothing launched)."""
    n_cols = int(n_cols)
    if store.dim() != 2 or not 0 <= n_cols <= store.shape[1]:
        raise ValueError(f"store: expected (K, at least {n_cols}), got {tuple(store.shape)}")
    if n_cols > ERR_MAX_COLS:
        raise ValueError(f"store: {n_cols} columns (at most {ERR_MAX_COLS})")
    if store.shape[1] > 0 and store.stride(1) != 1:
        raise ValueError("store: the rows of the error store must be contiguous")
    if q.dim() != 1 or not 1 <= q.numel() <= ERR_MAX_QUANTILES:
        raise ValueError(f"q: expected 1 to {ERR_MAX_QUANTILES} quantiles in one dimension, got {tuple(q.shape)}")
    if not (isinstance(store, torch.Tensor) and store.is_cuda and store.dtype == F32):
        raise _lib.PoseKernelError("store: expected a float32 CUDA(HIP) tensor; the hot path has no CPU implementation")
    q = _chk(q, F64, "q")
    K, Q = int(store.shape[0]), int(q.numel())
    order = torch.zeros(K, Q, 2, dtype=F32, device=store.device)
    summary = torch.zeros(K, 4, dtype=F64, device=store.device)
    _call_if(K * n_cols, "pk_kpt_error_quantiles", store, int(store.stride(0)), n_cols, K, q, Q, order, summary, stream_ptr())
    return order, summary


# ------------------------------------------------------------------------------------------------ occlusion sensitivity
BF16 = torch.bfloat16
OCCLUSION_MEASURES = {"sum": 0, "max": 1, "shift": 2}


def occlusion_positions(extent, patch, stride):
    """Patch positions along one axis (pk_occlusion_positions; host only): len(range(0, extent - patch, stride)), the reference's grid --
    the position extent - patch itself is not taken.  0 when extent <= patch."""
    n = _lib.lib.pk_occlusion_positions(int(extent), int(patch), int(stride))
    if n < 0:
        raise _lib.PoseKernelError(f"pk_occlusion_positions failed (code {n}): {_lib.lib.pk_last_error_string().decode()}")
    return n


def occlusion_grid(H, W, patch, stride):
    """(ny, nx) of an (H, W) image; an empty grid is an error that names the rule."""
    ny, nx = occlusion_positions(H, patch, stride), occlusion_positions(W, patch, stride)
    if ny == 0 or nx == 0:
        raise _lib.PoseKernelError(f"occlusion grid: no patch position: rows and columns start at range(0, extent - patch, stride), which is "
                                   f"empty for H={int(H)} W={int(W)} patch={int(patch)}")
    return ny, nx


def occlude_batch(x, patch, stride, first=0, n=None, fill=None, out=None):
    """Occluded copies first .. first + n - 1 of one packed image (pk_occlude_batch; no synchronisation).  x (H,W,8) or (1,H,W,8) bf16, the
    stem's layout; -> (n,H,W,8) bf16, or `out` when given (contiguous, at least n copies: its first n are written and returned).  Copy
    p = a nx + b has rows a stride .. a stride + patch - 1 and columns b stride .. b stride + patch - 1 replaced by `fill`: None = 0 in
    normalised space, or three floats per channel, rounded to bf16 as the input conversion rounds.  n = None: all from `first` on."""
    x = _chk(x, BF16, "x")
    if x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3 or x.shape[-1] != 8:
        raise _lib.PoseKernelError(f"occlude_batch: x {tuple(x.shape)} is not the packed image (H, W, 8) or (1, H, W, 8)")
    H, W = int(x.shape[0]), int(x.shape[1])
    ny, nx = occlusion_grid(H, W, patch, stride)
    first = int(first)
    n = ny * nx - first if n is None else int(n)
    if first < 0 or n < 1 or first + n > ny * nx:
        raise _lib.PoseKernelError(f"occlude_batch: copies {first} .. {first + n - 1} of {ny * nx} ({ny} x {nx} positions)")
    fill_ptr = None
    if fill is not None:
        fill = np.ascontiguousarray(np.asarray(fill, np.float32).reshape(-1))
        if fill.size != 3:
            raise _lib.PoseKernelError(f"occlude_batch: fill takes three floats, one per channel, got {fill.size}")
        fill_ptr = fill.ctypes.data                               # read before the call returns; carried in the launch
    if out is None:
        out = torch.empty(n, H, W, 8, dtype=BF16, device=x.device)
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == BF16 and out.is_contiguous() and out.dim() == 4
                and tuple(out.shape[1:]) == (H, W, 8) and out.shape[0] >= n):
            raise _lib.PoseKernelError(f"occlude_batch: out must be a contiguous bf16 device tensor (at least {n}, {H}, {W}, 8)")
        out = out[:n]
    call("pk_occlude_batch", x, out, H, W, int(patch), int(stride), first, n, fill_ptr, stream_ptr())
    return out


def heatmap_summary(heatmaps, out=None):
    """(..., h, w) -> (..., 4) float64: sum, max, argmax x, argmax y of every map in one pass (pk_heatmap_summary; no synchronisation).  fp32;
    a bf16 input is widened first.  The sum is taken in a fixed order and the first of equal maxima wins.  `out`: a contiguous float64
    device tensor of that shape to write into (a slice of a larger table)."""
    if isinstance(heatmaps, torch.Tensor) and heatmaps.dtype == BF16:
        heatmaps = heatmaps.float()
    hm = _chk(heatmaps, name="heatmaps")
    if hm.dim() < 2:
        raise _lib.PoseKernelError(f"heatmap_summary: heatmaps {tuple(hm.shape)} are not (..., h, w)")
    lead, h, w = tuple(hm.shape[:-2]), int(hm.shape[-2]), int(hm.shape[-1])
    M = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if out is None:
        out = torch.empty(*lead, 4, dtype=F64, device=hm.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == F64 and out.is_contiguous() and tuple(out.shape) == lead + (4,)):
        raise _lib.PoseKernelError(f"heatmap_summary: out must be a contiguous float64 device tensor {lead + (4,)}")
    _call_if(M * h * w, "pk_heatmap_summary", hm, out, M, h, w, stream_ptr())
    return out


def occlusion_paint(base, table, H, W, patch, stride, measure="sum"):
    """The reference's sensitivity map of every joint from the score table (pk_occlusion_paint; one launch, no synchronisation).  base (K,4)
    and table (P,K,4) or (ny,nx,K,4) float64 rows of `heatmap_summary` -> (K,H,W) float64: pixel (y, x) takes the value of the last patch
    the reference's loops write there, 0 where none does.  measure 'sum': base.sum - sum; 'max': base.max - max; 'shift': the distance of
    the argmax from the un-occluded one, in heat pixels."""
    if measure not in OCCLUSION_MEASURES:
        raise _lib.PoseKernelError(f"occlusion_paint: measure {measure!r} (one of {', '.join(OCCLUSION_MEASURES)})")
    ny, nx = occlusion_grid(H, W, patch, stride)
    base, table = _chk(base, F64, "base"), _chk(table, F64, "table")
    K = int(base.shape[0]) if base.dim() == 2 else -1
    if K < 1 or tuple(base.shape) != (K, 4) or tuple(table.shape) not in ((ny * nx, K, 4), (ny, nx, K, 4)):
        raise _lib.PoseKernelError(f"occlusion_paint: base (K,4) and table ({ny * nx},K,4) for {ny} x {nx} positions, got {tuple(base.shape)}, "
                                   f"{tuple(table.shape)}")
    maps = torch.empty(K, int(H), int(W), dtype=F64, device=base.device)
    call("pk_occlusion_paint", base, table, maps, OCCLUSION_MEASURES[measure], K, int(H), int(W), int(patch), int(stride), stream_ptr())
    return maps


# ------------------------------------------------------------------------------------------------ ensembles
ENSEMBLE_POINT_COLUMNS = ("n", "mean_x", "mean_y", "var_x", "var_y", "cov_xy", "axis_major_sq", "axis_minor_sq", "conf_mean", "conf_std",
                          "conf_min", "agreement")


def _ddof(who, ddof):
    if ddof not in (0, 1):
        raise _lib.PoseKernelError(f"{who}: ddof {ddof!r} (0 or 1)")
    return int(ddof)


def ensemble_moments(stack, ddof=0, out=None):
    """(S, ...) fp32 -> mean, std (...) fp32 over the S members, per element in float64 in ascending member order (pk_ensemble_moments; one
    launch, no synchronisation).  ddof 0 is np.std.  The stack may be a view whose member stride exceeds the member's size (a slice of a
    wider buffer); each member itself must be contiguous.  `out`: a pair of contiguous fp32 device tensors (...) to write into."""
    ddof = _ddof("ensemble_moments", ddof)
    if not (isinstance(stack, torch.Tensor) and stack.is_cuda):
        raise _lib.PoseKernelError("stack: expected a CUDA(HIP) tensor; the hot path has no CPU implementation")
    if stack.dtype != F32:
        raise _lib.PoseKernelError(f"stack: expected {F32}, got {stack.dtype}")
    if stack.dim() < 1:
        raise _lib.PoseKernelError(f"ensemble_moments: stack {tuple(stack.shape)} is not (S, ...)")
    S, rest = int(stack.shape[0]), tuple(stack.shape[1:])
    L = int(np.prod(rest, dtype=np.int64)) if rest else 1
    if S < 1 + ddof:
        raise _lib.PoseKernelError(f"ensemble_moments: {S} members with ddof={ddof} (at least {1 + ddof})")
    if L and not (stack[0].is_contiguous() and (S == 1 or stack.stride(0) >= L)):
        stack = stack.contiguous()
    stride = int(stack.stride(0)) if S > 1 and L else max(L, 1)
    if out is None:
        mean, std = torch.empty(rest, dtype=F32, device=stack.device), torch.empty(rest, dtype=F32, device=stack.device)
    else:
        mean, std = out
        for t in (mean, std):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F32 and t.is_contiguous() and tuple(t.shape) == rest):
                raise _lib.PoseKernelError(f"ensemble_moments: out must be two contiguous fp32 device tensors {rest}")
    _call_if(L, "pk_ensemble_moments", stack, stride, S, L, ddof, mean, std, stream_ptr())
    return mean, std


def ensemble_points(coords, conf=None, centre=None, min_conf=0.0, radius=1.0, ddof=0, out=None):
    """coords (S,M,2) fp32, conf (S,M) fp32 or None, centre (M,2) float64 or None -> (M,12) float64, the columns of
    ENSEMBLE_POINT_COLUMNS (pk_ensemble_points; one launch, no synchronisation): the number of valid members (finite, conf >= min_conf),
    their mean position, variances and covariance, the squared semi-axes of the 1-sigma ellipse, mean / std / min of conf, and how many
    lie within `radius` of `centre` (None: of the mean).  Fewer than 1 + ddof valid members: a row of zeros."""
    ddof = _ddof("ensemble_points", ddof)
    coords = _chk(coords, name="coords")
    if coords.dim() != 3 or coords.shape[-1] != 2:
        raise _lib.PoseKernelError(f"ensemble_points: coords {tuple(coords.shape)} are not (S, M, 2)")
    S, M = int(coords.shape[0]), int(coords.shape[1])
    if conf is not None:
        conf = _chk(conf, name="conf")
        if tuple(conf.shape) != (S, M):
            raise _lib.PoseKernelError(f"ensemble_points: conf {tuple(conf.shape)} is not ({S}, {M})")
    if centre is not None:
        centre = _chk(centre, F64, "centre")
        if tuple(centre.shape) != (M, 2):
            raise _lib.PoseKernelError(f"ensemble_points: centre {tuple(centre.shape)} is not ({M}, 2)")
    radius = float(radius)
    if not (radius >= 0.0 and math.isfinite(radius)):
        raise _lib.PoseKernelError(f"ensemble_points: radius {radius} (finite, at least 0)")
    if S < 1:
        raise _lib.PoseKernelError("ensemble_points: no members")
    if out is None:
        out = torch.empty(M, len(ENSEMBLE_POINT_COLUMNS), dtype=F64, device=coords.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == F64 and out.is_contiguous()
              and tuple(out.shape) == (M, len(ENSEMBLE_POINT_COLUMNS))):
        raise _lib.PoseKernelError(f"ensemble_points: out must be a contiguous float64 device tensor ({M}, {len(ENSEMBLE_POINT_COLUMNS)})")
    _call_if(M, "pk_ensemble_points", coords, conf, centre, out, S, M, float(min_conf), radius, ddof, stream_ptr())
    return out


# ------------------------------------------------------------------------------------------------ gradient attribution
STEM_DGRAD_MAX_COUT = _lib.CONSTANTS["PK_STEM_DGRAD_MAX_COUT"]


def stem_dgrad(g, w_packed, in_hw, c_real=3):
    """Data gradient of the stem's 3x3, stride-2, pad-1 conv (pk_stem_dgrad; one launch, no synchronisation).  g (B,Ho,Wo,Cout) bf16;
    w_packed [Cout][9][8] bf16, the FORWARD weight pack; in_hw = (Hs, Ws) -> dx (B,Hs,Ws,8) bf16, the packed pixel's gradient: fp32 sums,
    taps ascending then output channels ascending, one rounding; channels >= c_real exactly 0."""
    g, w_packed = _chk(g, BF16, "g"), _chk(w_packed, BF16, "w_packed")
    Hs, Ws = int(in_hw[0]), int(in_hw[1])
    if g.dim() != 4:
        raise _lib.PoseKernelError(f"stem_dgrad: g {tuple(g.shape)} is not (B, Ho, Wo, Cout)")
    B, Ho, Wo, Cout = (int(s) for s in g.shape)
    if Cout % 8 or not 0 < Cout <= STEM_DGRAD_MAX_COUT:
        raise _lib.PoseKernelError(f"stem_dgrad: Cout={Cout} (a multiple of 8 up to {STEM_DGRAD_MAX_COUT})")
    if tuple(w_packed.shape) != (Cout, 9, 8):
        raise _lib.PoseKernelError(f"stem_dgrad: w_packed {tuple(w_packed.shape)} is not the forward pack ({Cout}, 9, 8)")
    if not 1 <= int(c_real) <= 8:
        raise _lib.PoseKernelError(f"stem_dgrad: c_real={c_real} (1 to 8)")
    if Hs < 1 or Ws < 1 or (Ho, Wo) != ((Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1):
        raise _lib.PoseKernelError(f"stem_dgrad: g is {Ho} x {Wo}, a 3x3 stride-2 pad-1 conv of {Hs} x {Ws} gives "
                                   f"{(Hs - 1) // 2 + 1} x {(Ws - 1) // 2 + 1}")
    dx = torch.empty(B, Hs, Ws, 8, dtype=BF16, device=g.device)
    _call_if(B, "pk_stem_dgrad", g, w_packed, dx, B, Hs, Ws, Ho, Wo, Cout, int(c_real), stream_ptr())
    return dx


def _packed_grad(g, who):
    g = _chk(g, BF16, "g")
    if g.dim() == 3:
        g = g[None]
    if g.dim() != 4 or g.shape[-1] != 8:
        raise _lib.PoseKernelError(f"{who}: g {tuple(g.shape)} is not a packed gradient (B, H, W, 8) or (H, W, 8)")
    return g


def saliency_reduce(g, c_real=3):
    """Packed gradient (B,H,W,8) bf16 -> (B,H,W) fp32: max over the c_real real channels of |g| (pk_saliency_reduce; exact, one launch, no
    synchronisation).  A NaN in a real channel gives NaN, as torch.max does."""
    g = _packed_grad(g, "saliency_reduce")
    if not 1 <= int(c_real) <= 8:
        raise _lib.PoseKernelError(f"saliency_reduce: c_real={c_real} (1 to 8)")
    B, H, W = (int(s) for s in g.shape[:3])
    out = torch.empty(B, H, W, dtype=F32, device=g.device)
    _call_if(B * H * W, "pk_saliency_reduce", g, out, B, H, W, int(c_real), stream_ptr())
    return out


def packed_grad_to_nchw(g, channels=3):
    """Packed gradient (B,H,W,Cpad) bf16 -> (B,channels,H,W) fp32 (pk_nhwc_bf16_to_nchw_f32: exact, the backward of the input pack)."""
    g = _chk(g, BF16, "g")
    C = int(channels)
    if g.dim() != 4 or g.shape[-1] % 8 or not 1 <= C <= g.shape[-1]:
        raise _lib.PoseKernelError(f"packed_grad_to_nchw: g {tuple(g.shape)} is not (B, H, W, Cpad) with Cpad a multiple of 8 and {C} <= Cpad")
    B, H, W, Cp = (int(s) for s in g.shape)
    out = torch.empty(B, C, H, W, dtype=F32, device=g.device)
    _call_if(B * H * W, "pk_nhwc_bf16_to_nchw_f32", g, out, B, C, H, W, Cp, stream_ptr())
    return out


def grad_cam(activation, gradient, c_used=None):
    """Grad-CAM of every sample (pk_gradcam; two launches, no synchronisation).  activation and gradient (B,h,w,C) bf16 in the op layer's
    layout; channels >= c_used (a padded twin's) are ignored.  Per sample, in float64: weights = mean of the gradient over the pixels;
    raw = relu(sum_c weights[c] activation[..., c]); cam = (raw - min raw) / (max(raw - min raw) + 1e-8).
    -> cam (B,h,w) fp32, weights (B,c_used) fp32, range (B,2) float64 = min and max of raw (to undo the normalisation).  A NaN anywhere in
    a sample makes that sample's map NaN."""
    A, G = _chk(activation, BF16, "activation"), _chk(gradient, BF16, "gradient")
    if A.dim() != 4 or tuple(A.shape) != tuple(G.shape) or A.shape[-1] % 8:
        raise _lib.PoseKernelError(f"grad_cam: activation {tuple(A.shape)} and gradient {tuple(G.shape)} must both be (B, h, w, C), C a multiple of 8")
    B, h, w, C = (int(s) for s in A.shape)
    c_used = C if c_used is None else int(c_used)
    if not 1 <= c_used <= C:
        raise _lib.PoseKernelError(f"grad_cam: c_used={c_used} (1 to C={C})")
    cam = torch.empty(B, h, w, dtype=F32, device=A.device)
    weights = torch.empty(B, c_used, dtype=F32, device=A.device)
    rng = torch.empty(B, 2, dtype=F64, device=A.device)
    if B * h * w:
        n = _lib.lib.pk_gradcam_ws_floats(B, h, w, c_used)
        if n <= 0:
            raise _lib.PoseKernelError(f"pk_gradcam_ws_floats failed (code {n}): {_lib.lib.pk_last_error_string().decode()}")
        ws = torch.empty(n // 2, dtype=F64, device=A.device)
        call("pk_gradcam", A, G, ws, cam, weights, rng, B, h, w, C, c_used, stream_ptr())
    return cam, weights, rng


# ------------------------------------------------------------------------------------------------ overlays
U8 = torch.uint8


def _chk_images(images):
    """(N,H,W,3) uint8 device batch that the drawing kernels change IN PLACE (so no .contiguous() copy: it must be contiguous already)."""
    images = _chk(images, U8, "images")
    if images.dim() != 4 or images.shape[-1] != 3:
        raise _lib.PoseKernelError(f"images: expected (N, H, W, 3), got {tuple(images.shape)}")
    return images


def draw_shapes(images, poses=None, scores=None, image_index=None, limbs=None, colors=None, boxes=None, box_image_index=None,
                box_color=(0, 255, 0), box_thickness=2, score_threshold=0.3, point_radius=4, line_thickness=2):
    """Skeletons and boxes rasterised IN PLACE on a contiguous (N,H,W,3) uint8 batch, one launch (pk_draw_shapes).  poses (P,K,2) image
    pixels, scores (P,K), image_index (P,) int32 non-decreasing, limbs (L,2) int32, colors (C,3) uint8 in the image's channel order;
    boxes (Q,4) x1 y1 x2 y2 with box_image_index (Q,) int32 non-decreasing.  Returns `images`."""
    if not (isinstance(images, torch.Tensor) and images.is_contiguous()):
        raise _lib.PoseKernelError("images: expected a contiguous CUDA(HIP) uint8 tensor (drawn in place)")
    images = _chk_images(images)
    N, H, W, _ = images.shape
    P = K = L = C = Q = 0
    if poses is not None:
        poses, image_index = _chk(poses, name="poses"), _chk(image_index, I32, "image_index")
        P, K = int(poses.shape[0]), int(poses.shape[1])
        scores = _chk(scores, name="scores")
        colors = _chk(colors, U8, "colors")
        C = int(colors.shape[0])
        if tuple(poses.shape) != (P, K, 2) or tuple(scores.shape) != (P, K) or image_index.numel() != P or tuple(colors.shape) != (C, 3):
            raise _lib.PoseKernelError("draw_shapes: poses (P,K,2), scores (P,K), image_index (P,), colors (C,3)")
        if limbs is not None and limbs.numel():
            limbs = _chk(limbs, I32, "limbs")
            L = int(limbs.shape[0])
            if tuple(limbs.shape) != (L, 2):
                raise _lib.PoseKernelError("draw_shapes: limbs (L,2)")
        else:
            limbs = None
    if boxes is not None:
        boxes, box_image_index = _chk(boxes, name="boxes"), _chk(box_image_index, I32, "box_image_index")
        Q = int(boxes.shape[0])
        if tuple(boxes.shape) != (Q, 4) or box_image_index.numel() != Q:
            raise _lib.PoseKernelError("draw_shapes: boxes (Q,4), box_image_index (Q,)")
    b0, b1, b2 = (int(c) for c in box_color)
    _call_if(N * H * W, "pk_draw_shapes", images, N, H, W, poses if P else None, scores if P else None, image_index if P else None, P, K,
             limbs if P else None, L if P else 0, colors if P else None, C, boxes if Q else None, box_image_index if Q else None, Q, b0, b1, b2,
             int(box_thickness), float(score_threshold), int(point_radius), int(line_thickness), stream_ptr())
    return images


def heatmap_overlay(images, heatmaps, alpha, lut, want_index=False):
    """The heatmap overlay blended IN PLACE into a contiguous (N,H,W,3) uint8 batch (pk_heatmap_overlay): heatmaps (N,K,h,w) fp32,
    lut (256,3) uint8 in the image's channel order.  Returns the (N,H,W) uint8 colour-index plane if asked for, else None."""
    if not (isinstance(images, torch.Tensor) and images.is_contiguous()):
        raise _lib.PoseKernelError("images: expected a contiguous CUDA(HIP) uint8 tensor (drawn in place)")
    images, heatmaps, lut = _chk_images(images), _chk(heatmaps, name="heatmaps"), _chk(lut, U8, "lut")
    N, H, W, _ = images.shape
    if heatmaps.dim() != 4 or heatmaps.shape[0] != N or tuple(lut.shape) != (256, 3):
        raise _lib.PoseKernelError(f"heatmap_overlay: heatmaps (N,K,h,w) for N = {N} images and a (256,3) lut, got {tuple(heatmaps.shape)}, {tuple(lut.shape)}")
    _, K, h, w = heatmaps.shape
    index = torch.empty(N, H, W, dtype=U8, device=images.device) if want_index else None
    if N * H * W == 0:
        return index
    ws = torch.empty(max(1, _lib.lib.pk_heatmap_overlay_ws_floats(N, K, h, w, H, W)), dtype=F32, device=images.device)
    call("pk_heatmap_overlay", images, heatmaps, float(alpha), lut, index, ws, N, K, h, w, H, W, stream_ptr())
    return index


def heatmap_overlay_patches(images, heatmaps, image_index, matrices, alpha, lut, want_index=False, want_cover=False):
    """One heatmap stack per person, each blended IN PLACE where its crop lies in its frame (pk_heatmap_overlay_patches): images a
    contiguous (N,H,W,3) uint8 batch, heatmaps (P,K,h,w) fp32, image_index (P,) the frame of each patch, non-decreasing and in [0, N),
    matrices (P,6) or (P,2,3) float64, frame pixels -> heat-map pixels.  The index and the matrices are checked here, on the host (the
    kernel trusts them), so they are taken as host data; a device tensor is copied back first.  P = 0 or an empty batch launches
    nothing.  Returns (index, cover): the (N,H,W) uint8 colour-index plane (0 where uncovered) and the count of covering patches
    (saturating at 255), each None unless asked for."""
    if not (isinstance(images, torch.Tensor) and images.is_contiguous()):
        raise _lib.PoseKernelError("images: expected a contiguous CUDA(HIP) uint8 tensor (drawn in place)")
    images, heatmaps, lut = _chk_images(images), _chk(heatmaps, name="heatmaps"), _chk(lut, U8, "lut")
    N, H, W, _ = images.shape
    if heatmaps.dim() != 4 or tuple(lut.shape) != (256, 3):
        raise _lib.PoseKernelError(f"heatmap_overlay_patches: heatmaps (P,K,h,w) and a (256,3) lut, got {tuple(heatmaps.shape)}, {tuple(lut.shape)}")
    P, K, h, w = heatmaps.shape
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)     # noqa: E731
    idx, mats = host(image_index).reshape(-1), host(matrices)
    if idx.size != P or mats.size != 6 * P:
        raise _lib.PoseKernelError(f"heatmap_overlay_patches: {P} patches need image_index ({P},) and matrices ({P},6), got {idx.shape}, {mats.shape}")
    if idx.size and idx.dtype.kind not in "iu":
        raise _lib.PoseKernelError(f"heatmap_overlay_patches: image_index must be integer, got {idx.dtype}")
    idx, mats = idx.astype(np.int64), np.ascontiguousarray(mats, np.float64).reshape(P, 6)
    if P and (idx.min() < 0 or idx.max() >= N or np.any(np.diff(idx) < 0)):
        raise _lib.PoseKernelError(f"heatmap_overlay_patches: image_index must be non-decreasing with every entry in [0, {N}), got {idx.tolist()}")
    if not np.all(np.isfinite(mats)):
        raise _lib.PoseKernelError("heatmap_overlay_patches: a matrix entry is not finite")
    launch = N * H * W > 0 and P > 0
    plane = torch.empty if launch else torch.zeros         # the kernel writes every pixel of both planes
    index = plane(N, H, W, dtype=U8, device=images.device) if want_index else None
    cover = plane(N, H, W, dtype=U8, device=images.device) if want_cover else None
    if not launch:
        return index, cover
    n_ws = _lib.lib.pk_heatmap_overlay_patches_ws_floats(P, K, h, w)
    ws = torch.empty(max(1, n_ws), dtype=F32, device=images.device)
    call("pk_heatmap_overlay_patches", images, heatmaps, torch.from_numpy(idx.astype(np.int32)).to(images.device),
         torch.from_numpy(mats).to(images.device), float(alpha), lut, index, cover, ws, N, P, K, h, w, H, W, stream_ptr())
    return index, cover


# ------------------------------------------------------------------------------------------------ optimiser
def adamw_step(param, grad, exp_avg, exp_avg_sq, flags, param_bf16, lr_dev, step_dev, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    call("pk_adamw_step", param, grad, exp_avg, exp_avg_sq, flags, param_bf16, param.numel(), lr_dev, step_dev, float(beta1), float(beta2),
         float(eps), float(weight_decay), float(grad_scale), stream_ptr())


# Guarded step: grad_sumsq -> grad_guard_finalize -> adamw_step_guarded on the current stream.  The norm and the skip decision are
# written to `guard_state` on the device and read there by the update; nothing here reads them back.
GUARD_STATE_WORDS = 4          # {float norm, float coef, int32 skipped_last, int32 skipped_total}


def grad_sumsq_partials(n):
    """Workgroups pk_grad_sumsq launches for n elements (a function of n only): `partials` is a (that many, 2) float64 tensor."""
    k = _lib.lib.pk_grad_sumsq_partials(int(n))
    if k <= 0:
        raise _lib.PoseKernelError(f"pk_grad_sumsq_partials failed: {_lib.lib.pk_last_error_string().decode()}")
    return k


def _chk_guard_state(guard_state):
    if _chk(guard_state, I32, "guard_state").numel() != GUARD_STATE_WORDS:
        raise _lib.PoseKernelError(f"guard_state: expected {GUARD_STATE_WORDS} int32 words, got {guard_state.numel()}")


def _chk_partials(partials):
    if not (isinstance(partials, torch.Tensor) and partials.is_cuda and partials.dtype == torch.float64 and partials.dim() == 2
            and partials.shape[1] == 2 and partials.is_contiguous()):
        raise _lib.PoseKernelError("partials: expected a contiguous (n_partials, 2) float64 CUDA(HIP) tensor")


def grad_sumsq(grad, flags, partials):
    """partials[b] = {fp64 sum of grad^2 over workgroup b's share of the elements with flag bit1, 1.0 if one of them is inf/NaN else 0.0}."""
    _chk_partials(partials)
    if _chk(flags, torch.uint8, "flags").numel() != _chk(grad, name="grad").numel():
        raise _lib.PoseKernelError(f"grad_sumsq: {grad.numel()} gradients but {flags.numel()} flags")
    call("pk_grad_sumsq", grad, flags, grad.numel(), partials, partials.shape[0], stream_ptr())
    return partials


def grad_guard_finalize(partials, grad_scale, max_norm, guard_state, step_dev):
    _chk_partials(partials)
    _chk_guard_state(guard_state)
    call("pk_grad_guard_finalize", partials, partials.shape[0], float(grad_scale), float(max_norm), guard_state,
         _chk(step_dev, I32, "step_dev"), stream_ptr())


def adamw_step_guarded(param, grad, exp_avg, exp_avg_sq, flags, param_bf16, lr_dev, step_dev, beta1, beta2, eps, weight_decay, guard_state,
                       grad_scale=1.0):
    _chk_guard_state(guard_state)
    call("pk_adamw_step_guarded", param, grad, exp_avg, exp_avg_sq, flags, param_bf16, param.numel(), lr_dev, step_dev, float(beta1),
         float(beta2), float(eps), float(weight_decay), float(grad_scale), guard_state, stream_ptr())


def adamw_step_ema(param, grad, exp_avg, exp_avg_sq, flags, param_bf16, lr_dev, step_dev, beta1, beta2, eps, weight_decay, guard_state, ema,
                   ema_decay, grad_scale=1.0):
    """The plain (guard_state None) or guarded update, and in the same pass ema += (1 - d_t) * (param_new - ema) on the elements that were
    updated; d_t = min(ema_decay, (1 + t) / (10 + t)) is worked out on the device from step_dev.  A skipped step leaves `ema` alone too."""
    if guard_state is not None:
        _chk_guard_state(guard_state)
    if _chk(ema, name="ema").numel() != param.numel() or not ema.is_contiguous():
        raise _lib.PoseKernelError(f"adamw_step_ema: ema must be a contiguous buffer of {param.numel()} floats (updated in place)")
    call("pk_adamw_step_ema", param, grad, exp_avg, exp_avg_sq, flags, param_bf16, param.numel(), lr_dev, step_dev, float(beta1),
         float(beta2), float(eps), float(weight_decay), float(grad_scale), guard_state, ema, float(ema_decay), stream_ptr())


# ------------------------------------------------------------------------------------------------ per-tensor statistics
# pk_tensor_stats: a segmented reduction over a flat fp32 buffer in two launches on the current stream; one 64-byte record per tensor.
TENSOR_STATS_RECORD = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("sumabs", "<f8"), ("min", "<f4"), ("max", "<f4"), ("n", "<i8"),
                                ("nonfinite", "<i8"), ("small", "<i8"), ("zero", "<i8")])
assert TENSOR_STATS_RECORD.itemsize == _lib.CONSTANTS["PK_TENSOR_STATS_RECORD_BYTES"]
LATCH_STATE_WORDS = 4          # {int32 events, first offending tensor, last offending tensor, offending tensors}


def _query(name, *args):
    k = getattr(_lib.lib, name)(*args)
    if k <= 0:
        raise _lib.PoseKernelError(f"{name} failed: {_lib.lib.pk_last_error_string().decode()}")
    return k


def tensor_stats_chunk_elems():
    return _query("pk_tensor_stats_chunk_elems")


def tensor_stats_plan_host(offsets, counts):
    """The launch plan of a segment table, built by the library on the host: (plan as a uint8 numpy array, n_items)."""
    seg = np.ascontiguousarray(np.stack([np.asarray(offsets, np.int64), np.asarray(counts, np.int64)], axis=1))
    if seg.ndim != 2 or seg.shape[0] == 0:
        raise _lib.PoseKernelError("tensor_stats_plan_host: the segment table is empty")
    n_items = _query("pk_tensor_stats_plan", seg.ctypes.data, seg.shape[0], None, 0)
    plan = np.zeros(_query("pk_tensor_stats_plan_bytes", n_items, seg.shape[0]) // 8, np.int64)
    if _query("pk_tensor_stats_plan", seg.ctypes.data, seg.shape[0], plan.ctypes.data, plan.nbytes) != n_items:
        raise _lib.PoseKernelError("pk_tensor_stats_plan: the item count changed between two calls")
    return plan.view(np.uint8), n_items


class TensorStatsPlan:
    """Static device memory of one segment table: the uploaded plan, the partial workspace and the records.  Built once (one
    host-to-device copy), so that `tensor_stats` allocates and copies nothing and can be captured."""

    def __init__(self, offsets, counts, device):
        self.offsets, self.counts = [int(o) for o in offsets], [int(c) for c in counts]
        self.n_tensors = len(self.offsets)
        plan, self.n_items = tensor_stats_plan_host(self.offsets, self.counts)
        self.extent = max(o + c for o, c in zip(self.offsets, self.counts))
        self.plan = torch.from_numpy(plan.copy()).to(device)
        self.ws = torch.empty(_query("pk_tensor_stats_ws_bytes", self.n_items, self.n_tensors), dtype=torch.uint8, device=device)
        self.records = torch.zeros(self.n_tensors * TENSOR_STATS_RECORD.itemsize, dtype=torch.uint8, device=device)


def tensor_stats(plan, a, b=None, flags=None, tiny=0.0, records=None):
    """Records of `a` (or of a - b, rounded once to fp32) over `plan`'s tensors, elements with flag bit1 only when `flags` is given.
    Returns the records tensor (uint8, n_tensors x 64 bytes; `plan.records` unless another is passed).  No allocation, copy or sync."""
    if not isinstance(plan, TensorStatsPlan):
        raise _lib.PoseKernelError("tensor_stats: plan must be a TensorStatsPlan")
    for t, name, dt in ((a, "a", F32), (b, "b", F32), (flags, "flags", torch.uint8)):
        if t is None and name != "a":
            continue
        _chk(t, dt, name)
        if not t.is_contiguous() or t.numel() < plan.extent or t.device != plan.plan.device:
            raise _lib.PoseKernelError(f"tensor_stats: {name} must be a contiguous buffer of at least {plan.extent} elements on "
                                       f"{plan.plan.device}")
    records = plan.records if records is None else records
    if _chk(records, torch.uint8, "records").numel() != plan.records.numel() or not records.is_contiguous():
        raise _lib.PoseKernelError(f"tensor_stats: records must be {plan.records.numel()} contiguous bytes")
    call("pk_tensor_stats", a, b, flags, plan.plan, plan.n_tensors, plan.n_items, float(tiny), plan.ws, plan.ws.numel(), records,
         stream_ptr())
    return records


def tensor_stats_latch(records, n_tensors, latched, latch_state):
    """If any record counts a non-finite element: latched <- records, latch_state <- {events + 1, first, last, how many}; else nothing."""
    if _chk(latch_state, I32, "latch_state").numel() != LATCH_STATE_WORDS:
        raise _lib.PoseKernelError(f"latch_state: expected {LATCH_STATE_WORDS} int32 words, got {latch_state.numel()}")
    need = n_tensors * TENSOR_STATS_RECORD.itemsize
    if _chk(records, torch.uint8, "records").numel() != need or _chk(latched, torch.uint8, "latched").numel() != need:
        raise _lib.PoseKernelError(f"tensor_stats_latch: records and latched must be {need} bytes each")
    call("pk_tensor_stats_latch", records, int(n_tensors), latched, latch_state, stream_ptr())


def tensor_stats_records(records):
    """The records tensor as a numpy structured array (ONE device read)."""
    return records.cpu().numpy().view(TENSOR_STATS_RECORD)


def derive_tensor_stats(rec, scale=1.0):
    """The reported values of one raw record, in float64: the reference's mean / std / min / max / norm (std: population value, clamped
    at 0), abs_mean / abs_max, and the counts.  `scale` multiplies the linear quantities.  A tensor without a finite participating
    element has mean = std = nan.  Pure host arithmetic: `rec` is anything indexable by the record's field names."""
    n, bad = int(rec["n"]), int(rec["nonfinite"])
    m, s = n - bad, abs(float(scale))
    out = {"numel": n, "nonfinite": bad, "small": int(rec["small"])}
    sc = float(scale)
    lo, hi = float(rec["min"]) * sc, float(rec["max"]) * sc
    out["min"], out["max"] = (lo, hi) if sc >= 0 else (hi, lo)
    out["norm"] = s * math.sqrt(float(rec["sumsq"]))
    out["abs_max"] = max(abs(float(rec["min"])), abs(float(rec["max"]))) * s if m else 0.0
    if m == 0:
        out["mean"] = out["std"] = out["abs_mean"] = float("nan")
        return out
    mean = float(rec["sum"]) / m
    out["mean"] = mean * sc
    # E[x^2] - mean^2 cancels to rounding noise of either sign on a constant tensor: min == max says so exactly
    var = 0.0 if rec["min"] == rec["max"] else max(float(rec["sumsq"]) / m - mean * mean, 0.0)
    out["std"] = s * math.sqrt(var)
    out["abs_mean"] = s * float(rec["sumabs"]) / m
    return out


# ------------------------------------------------------------------------------------------------ activation statistics
# pk_activation_stats / pk_activation_quantiles: per-channel records, a 4096-bin table over the bf16 bit patterns and exact order
# statistics of an NHWC bf16 feature map, on the current stream; nothing is read back.
ACT_RECORD = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("min", "<f4"), ("max", "<f4"), ("n", "<i8"), ("n_zero", "<i8"),
                       ("n_negative", "<i8"), ("n_nonfinite", "<i8"), ("reserved", "<i8")])
assert ACT_RECORD.itemsize == _lib.CONSTANTS["PK_ACT_RECORD_BYTES"]
ACT_HIST_BINS = _lib.CONSTANTS["PK_ACT_HIST_BINS"]
ACT_MAX_QUANTILES = _lib.CONSTANTS["PK_ACT_MAX_QUANTILES"]
ACT_MAX_CHANNELS = _lib.CONSTANTS["PK_ACT_MAX_CHANNELS"]
_ACT_WS = {}           # (device, stream, entry) -> the largest workspace asked for so far


def _act_rows(x, c_used, who):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise _lib.PoseKernelError(f"{who}: x: expected a CUDA(HIP) tensor; the hot path has no CPU implementation")
    if x.dtype != BF16:
        raise _lib.PoseKernelError(f"{who}: x: expected {BF16}, got {x.dtype}")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"{who}: x: expected a non-empty (..., C) tensor, got {tuple(x.shape)}")
    C = int(x.shape[-1])
    if C % 8 or not 8 <= C <= ACT_MAX_CHANNELS:
        raise ValueError(f"{who}: x: {C} channels (a multiple of 8 from 8 to {ACT_MAX_CHANNELS})")
    c_used = C if c_used is None else int(c_used)
    if not 1 <= c_used <= C:
        raise ValueError(f"{who}: c_used={c_used} outside [1, {C}]")
    x = x.contiguous()
    return x, x.numel() // C, C, c_used


def _act_ws(x, entry, M, C):
    # one workspace per (device, stream, entry): launches on one stream are ordered, two streams must not share partials
    key = (x.device, stream_ptr(), entry)
    need = _query(f"pk_activation_{entry}_ws_bytes", M, C)
    ws = _ACT_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _ACT_WS[key] = torch.empty(need, dtype=torch.uint8, device=x.device)
    return ws


def activation_stats_blocks(M, C):
    """Workgroups of the partial kernel for an (M, C) map and the rows of one slab: the split that fixes the order of the sums."""
    return _query("pk_activation_stats_blocks", int(M), int(C)), _query("pk_activation_stats_slab", int(C))


def activation_stats(x, c_used=None, records=None, hist=None):
    """Per-channel records and the 4096-bin table of a device bf16 (..., C) tensor (pk_activation_stats; two launches on the current stream,
    no synchronisation).  Channels >= c_used are padding.  -> (records: uint8, c_used x 64 bytes, see ACT_RECORD; hist: (4096,) int64).
    With `records` and `hist` of an earlier call given, that call's numbers are added to in place (old + new per field, min / max
    combined): several batches of one layer."""
    x, M, C, c_used = _act_rows(x, c_used, "activation_stats")
    if (records is None) != (hist is None):
        raise ValueError("activation_stats: pass both records and hist of the earlier call, or neither")
    accumulate = records is not None
    if accumulate:
        if _chk(records, torch.uint8, "records").numel() != c_used * ACT_RECORD.itemsize or not records.is_contiguous():
            raise _lib.PoseKernelError(f"activation_stats: records must be {c_used * ACT_RECORD.itemsize} contiguous bytes")
        if _chk(hist, I64, "hist").numel() != ACT_HIST_BINS or not hist.is_contiguous():
            raise _lib.PoseKernelError(f"activation_stats: hist must be {ACT_HIST_BINS} contiguous int64 counts")
    else:
        records = torch.empty(c_used * ACT_RECORD.itemsize, dtype=torch.uint8, device=x.device)
        hist = torch.empty(ACT_HIST_BINS, dtype=I64, device=x.device)
    ws = _act_ws(x, "stats", M, C)
    call("pk_activation_stats", x, M, C, c_used, ws, ws.numel(), records, hist, 1 if accumulate else 0, stream_ptr())
    return records, hist


def activation_quantiles(x, hist, q, c_used=None):
    """Exact order statistics of the finite elements of the channels < c_used of x (pk_activation_quantiles; three launches on the current
    stream, no synchronisation).  hist: the table `activation_stats` returned for the same x and c_used.  q: up to 16 host floats in [0, 1].
    -> (Q,2) float32 on the device: v[lo], v[hi] around position q (n - 1) of the n values in ascending order; NaN when there is none."""
    x, M, C, c_used = _act_rows(x, c_used, "activation_quantiles")
    qs = np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1))
    if not 1 <= qs.size <= ACT_MAX_QUANTILES:
        raise ValueError(f"activation_quantiles: q: expected 1 to {ACT_MAX_QUANTILES} quantiles, got {qs.size}")
    if not bool(np.all((qs >= 0.0) & (qs <= 1.0))):
        raise ValueError(f"activation_quantiles: q: every quantile must lie in [0, 1], got {qs.tolist()}")
    if _chk(hist, I64, "hist").numel() != ACT_HIST_BINS or not hist.is_contiguous():
        raise _lib.PoseKernelError(f"activation_quantiles: hist must be {ACT_HIST_BINS} contiguous int64 counts")
    order = torch.empty(qs.size, 2, dtype=F32, device=x.device)
    ws = _act_ws(x, "quantiles", M, C)
    call("pk_activation_quantiles", x, M, C, c_used, hist, qs.ctypes.data, int(qs.size), ws, ws.numel(), order, stream_ptr())
    return order


def activation_records(records):
    """The records tensor as a numpy structured array (ONE device read)."""
    return records.cpu().numpy().view(ACT_RECORD)


def activation_bin_edges():
    """The 4097 edges of the table as float64: bin b holds lo[b] <= x < lo[b + 1], the same for every tensor.  Edge b is the smallest
    value of bin b -- the bf16 whose key is 16 b -- except inside the two NaN ranges at either end, where it is -inf / +inf."""
    keys = (np.arange(ACT_HIST_BINS + 1, dtype=np.int64) << 4)
    keys[-1] = 0xffff
    bits = np.where(keys & 0x8000, keys & 0x7fff, ~keys & 0xffff).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        edges = (bits << 16).view(np.float32).astype(np.float64)
    edges[np.isnan(edges) & (np.arange(ACT_HIST_BINS + 1) < ACT_HIST_BINS // 2)] = -np.inf
    edges[np.isnan(edges)] = np.inf
    return edges


# ------------------------------------------------------------------------------------------------ feature sheets, heat-map quality
# pk_gather_planes / pk_plane_sheet / pk_heatmap_quality: channel planes of a tapped map, a finished uint8 sheet of colour-mapped tiles and
# one float64 record per pair of maps, on the current stream; nothing is read back.
PANEL_MAX_TILES = _lib.CONSTANTS["PK_PANEL_MAX_TILES"]
PANEL_MAX_SIDE = _lib.CONSTANTS["PK_PANEL_MAX_SIDE"]
QUALITY_COLS = _lib.CONSTANTS["PK_QUALITY_COLS"]


def gather_planes(x, channels, sample=0, c_used=None):
    """Channels of one sample of an NHWC map as planes (pk_gather_planes; one launch, no synchronisation).  x (B,H,W,C) bf16, C a multiple
    of 8; channels (n,) int32 on the device -> (n,H,W) fp32, plane i = x[sample, :, :, channels[i]] widened.  A channel outside
    [0, c_used) gives a plane of NaN (the kernel reads nothing for it); callers check their list on the host before they upload it."""
    x, channels = _chk(x, BF16, "x"), _chk(channels, I32, "channels")
    if x.dim() != 4 or x.shape[-1] % 8 or x.numel() == 0:
        raise _lib.PoseKernelError(f"gather_planes: x {tuple(x.shape)} is not a non-empty (B, H, W, C) map with C a multiple of 8")
    B, H, W, C = (int(s) for s in x.shape)
    c_used = C if c_used is None else int(c_used)
    n = int(channels.numel())
    if channels.dim() != 1 or not 1 <= n <= PANEL_MAX_TILES:
        raise _lib.PoseKernelError(f"gather_planes: channels {tuple(channels.shape)} is not a list of 1 to {PANEL_MAX_TILES} entries")
    if not 0 <= int(sample) < B or not 1 <= c_used <= C:
        raise _lib.PoseKernelError(f"gather_planes: sample={sample} of {B}, c_used={c_used} of {C}")
    out = torch.empty(n, H, W, dtype=F32, device=x.device)
    call("pk_gather_planes", x, B, H, W, C, int(sample), channels, n, c_used, out, stream_ptr())
    return out


def plane_sheet_size(T, h, w, cols, zoom, pad):
    """(SH, SW) of a sheet of T tiles of h x w elements (pk_plane_sheet_size: host only); raises for what the library refuses."""
    SH, SW = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib.pk_plane_sheet_size(int(T), int(h), int(w), int(cols), int(zoom), int(pad), ctypes.addressof(SH), ctypes.addressof(SW))
    if rc != 0:
        raise _lib.PoseKernelError(f"pk_plane_sheet_size failed (code {rc}): {_lib.lib.pk_last_error_string().decode()}")
    return SH.value, SW.value


def plane_sheet(a, tiles, luts, b=None, cols=4, zoom=1, pad=2, background=(255, 255, 255)):
    """T colour-mapped tiles on one sheet (pk_plane_sheet; two launches, no synchronisation).  a (Na,h,w) fp32; b (Nb,h,w) fp32 or None;
    tiles (T,3) int32 on the device = {ia, ib or -1, ramp}: the tile shows a[ia], or |a[ia] - b[ib]|, scaled to its own range of finite
    values and looked up in luts[ramp]; luts (L,256,3) or (256,3) uint8 in the sheet's channel order.  Tile t sits at row t // cols,
    column t % cols, every element zoom x zoom pixels, pad pixels of `background` around each tile.  A tile that names a plane or a ramp
    that does not exist is background.  -> (sheet (SH,SW,3) uint8, ranges (T,2) fp32: lo, hi of each tile; +inf, -inf without a finite
    value, NaN for a refused tile)."""
    a, tiles, luts = _chk(a, name="a"), _chk(tiles, I32, "tiles"), _chk(luts, U8, "luts")
    if luts.dim() == 2:
        luts = luts[None]
    if a.dim() != 3 or a.numel() == 0 or tiles.dim() != 2 or tiles.shape[1] != 3 or luts.dim() != 3 or tuple(luts.shape[1:]) != (256, 3) \
            or luts.shape[0] < 1:
        raise _lib.PoseKernelError(f"plane_sheet: a (Na,h,w), tiles (T,3) and luts (L,256,3), got {tuple(a.shape)}, {tuple(tiles.shape)}, "
                                   f"{tuple(luts.shape)}")
    Na, h, w = (int(s) for s in a.shape)
    Nb = 0
    if b is not None:
        b = _chk(b, name="b")
        if b.dim() != 3 or tuple(b.shape[1:]) != (h, w) or b.shape[0] < 1:
            raise _lib.PoseKernelError(f"plane_sheet: b {tuple(b.shape)} is not (Nb, {h}, {w})")
        Nb = int(b.shape[0])
    T, L = int(tiles.shape[0]), int(luts.shape[0])
    SH, SW = plane_sheet_size(T, h, w, cols, zoom, pad)
    bg = [int(c) for c in background]
    if len(bg) != 3 or not all(0 <= c <= 255 for c in bg):
        raise _lib.PoseKernelError(f"plane_sheet: background {background} is not three bytes")
    sheet = torch.empty(SH, SW, 3, dtype=U8, device=a.device)
    ranges = torch.empty(T, 2, dtype=F32, device=a.device)
    call("pk_plane_sheet", a, Na, b, Nb, tiles, T, luts, L, ranges, sheet, h, w, int(cols), int(zoom), int(pad), bg[0], bg[1], bg[2], stream_ptr())
    return sheet, ranges


def heatmap_quality(pred, gt, out=None):
    """(..., h, w) predicted and target maps -> (..., 16) float64 records (pk_heatmap_quality; one launch, no synchronisation).  Columns:
    0, 1 sum p, sum g; 2 sum (p - g)^2; 3 max |p - g|; 4-6 max p, its x, its y (the first of equal maxima); 7-9 the same for g; 10-12
    sum (p - mean p)(g - mean g), sum (p - mean p)^2, sum (g - mean g)^2; 13, 14 the elements above half of both peaks, and of either;
    15 the elements left out because p or g is not finite.  Every sum in float64 in a fixed order.  `out`: a contiguous float64 device
    tensor of that shape to write into (a slice of a larger table)."""
    p, g = _chk(pred, name="pred"), _chk(gt, name="gt")
    if p.dim() < 2 or tuple(p.shape) != tuple(g.shape):
        raise _lib.PoseKernelError(f"heatmap_quality: pred {tuple(p.shape)} and gt {tuple(g.shape)} must both be (..., h, w)")
    lead, h, w = tuple(p.shape[:-2]), int(p.shape[-2]), int(p.shape[-1])
    M = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if out is None:
        out = torch.empty(*lead, QUALITY_COLS, dtype=F64, device=p.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == F64 and out.is_contiguous()
              and tuple(out.shape) == lead + (QUALITY_COLS,)):
        raise _lib.PoseKernelError(f"heatmap_quality: out must be a contiguous float64 device tensor {lead + (QUALITY_COLS,)}")
    _call_if(M * h * w, "pk_heatmap_quality", p, g, out, M, h, w, stream_ptr())
    return out
