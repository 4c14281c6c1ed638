"""Occlusion sensitivity on the device (rules: DESIGN.md, "Occlusion sensitivity").

The reference's `SensitivityAnalyzer.occlusion_sensitivity` (analysis/advanced_analysis.py:387-427) blanks one patch of the crop at a time,
runs a batch-1 forward and reads one heat-map sum back to the host -- 660 forwards and 661 synchronisations at 256 x 192 with patch 16 and
stride 8, for one joint.  In eval mode every sample of a batch is independent of the others and bit-reproducible, so here the occluded
copies are made in the stem's packed layout by one kernel per chunk (pk_occlude_batch), go through the model `batch_size` at a time, every
output map is reduced to its score by one kernel per chunk (pk_heatmap_summary), and one kernel paints the reference's map of EVERY joint
from the score table (pk_occlusion_paint).  Nothing is read back in between."""
import numpy as np
import torch

from .. import hipops, nnops

__all__ = ['SensitivityAnalyzer', 'occlusion_sensitivity_maps']


def _packed_image(image):
    """(1,3,H,W) or (3,H,W) fp32 normalised, or the packed (1,H,W,8) / (H,W,8) bf16 -> (1,H,W,8) bf16, packed once."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise TypeError("occlusion_sensitivity_maps: image must be a device tensor (the sweep has no CPU implementation)")
    if image.dtype == torch.bfloat16 and image.shape[-1] == 8 and image.dim() in (3, 4):
        image = image[None] if image.dim() == 3 else image
    elif image.dim() in (3, 4) and image.shape[-3] == 3:
        image = image[None] if image.dim() == 3 else image
    else:
        raise ValueError(f"occlusion_sensitivity_maps: image {tuple(image.shape)} is neither (1,3,H,W) / (3,H,W) nor the packed (1,H,W,8) bf16")
    if image.shape[0] != 1:
        raise ValueError(f"occlusion_sensitivity_maps: one image at a time, got a batch of {image.shape[0]}")
    return nnops.to_features(image)


@torch.no_grad()
def occlusion_sensitivity_maps(model, image, patch_size=16, stride=8, measure='sum', batch_size=256, fill=None):
    """The occlusion sensitivity maps of ALL joints from one batched sweep.

    image: (1,3,H,W) or (3,H,W) fp32 normalised device tensor, or the stem's packed (1,H,W,8) bf16.  Patch rows start at
    range(0, H - patch_size, stride), columns likewise (the reference's grid: the last position H - patch_size is not taken); copy
    a * nx + b has that patch replaced by `fill` (None: 0 in normalised space, as the reference does; or three floats per channel).
    measure: 'sum' = drop of the map's sum (the reference's), 'max' = drop of its peak (this project's keypoint score), 'shift' = distance
    in heat pixels the argmax moved.  The model must be in eval mode (batch statistics would couple the copies: RuntimeError otherwise).
    At most `batch_size` copies go through the model at a time; the result does not depend on it (the default is the measured one:
    DESIGN.md "Occlusion sensitivity", Cost).
    -> dict: maps (K,H,W) float64 on the device, each pixel holding the value of the last patch the reference's loops write there (0 where
    none does); base (K,4) and table (ny,nx,K,4) float64: sum, max, argmax x, argmax y of the un-occluded and of every occluded forward;
    grid (ny, nx).  No host synchronisation anywhere."""
    if model.training:
        raise RuntimeError("occlusion_sensitivity_maps needs eval mode: in training mode batch statistics would couple the occluded copies")
    if measure not in hipops.OCCLUSION_MEASURES:
        raise ValueError(f"measure must be one of {', '.join(hipops.OCCLUSION_MEASURES)}, got {measure!r}")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size {batch_size}")
    x = _packed_image(image)
    H, W = int(x.shape[1]), int(x.shape[2])
    ny, nx = hipops.occlusion_grid(H, W, patch_size, stride)
    P, step = ny * nx, min(int(batch_size), ny * nx)
    base = hipops.heatmap_summary(model(x)['heatmaps'])[0]
    K = int(base.shape[0])
    table = torch.empty(P, K, 4, dtype=torch.float64, device=x.device)
    chunk = torch.empty(step, H, W, 8, dtype=torch.bfloat16, device=x.device)
    for first in range(0, P, step):
        n = min(step, P - first)
        copies = hipops.occlude_batch(x, patch_size, stride, first, n, fill, out=chunk)
        hipops.heatmap_summary(model(copies)['heatmaps'], out=table[first:first + n])
    maps = hipops.occlusion_paint(base, table, H, W, patch_size, stride, measure)
    return {'maps': maps, 'base': base, 'table': table.view(ny, nx, K, 4), 'grid': (ny, nx)}


class SensitivityAnalyzer:
    """The reference's class (analysis/advanced_analysis.py), as far as it is ported: the occlusion map."""

    @staticmethod
    def occlusion_sensitivity(model, image, target_keypoint, patch_size=16, stride=8):
        """The reference's call: a numpy (H,W) float64 map of joint `target_keypoint`, the drop of that joint's heat-map sum under every
        patch.  Like the reference it puts the model into eval mode.  (`occlusion_sensitivity_maps` gives all joints for the same cost and
        keeps them on the device.)"""
        model.eval()
        device = next(model.parameters()).device
        maps = occlusion_sensitivity_maps(model, image.to(device), patch_size, stride)['maps']
        return maps[target_keypoint].cpu().numpy().astype(np.float64, copy=False)
