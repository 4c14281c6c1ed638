"""Predictive uncertainty on the device: stochastic-depth ensembles (rules: DESIGN.md, "Predictive uncertainty").

The reference's `UncertaintyAnalyzer.monte_carlo_dropout_uncertainty` (analysis/advanced_analysis.py:430-485) switches the nn.Dropout
modules to train mode, runs 30 batch-1 forwards, copies each to the host and takes np.mean / np.std.  Every nn.Dropout of its models has
p = 0 and DropPath is not an nn.Dropout, so its 30 forwards are identical and its std map is zero.  The stochastic layer these networks
do have is stochastic depth.  Here the S members are the rows of ONE batch: all DropPath multipliers are drawn in one launch, the eval-mode
forward takes them through `nnops.stochastic_depth`, and three kernels turn the stack into maps and per-joint numbers (pk_ensemble_moments,
pk_heatmap_summary, pk_ensemble_points).  Nothing is read back in between."""
import numpy as np
import torch

from .. import hipops, nnops
from .sensitivity import _packed_image

__all__ = ['UncertaintyAnalyzer', 'mc_uncertainty', 'stochastic_depth_draws']


def stochastic_depth_draws(model):
    """(n_draws, rate) of the model's backbone: the DropPath multipliers one forward takes per sample and the configured rate; (0, 0.0)
    for a model without a stochastic-depth layer (the HRNets)."""
    backbone = getattr(model, 'backbone', model)
    mods = [m for m in backbone.modules() if hasattr(m, 'n_draws')]
    if not mods or not hasattr(backbone, 'drop_path_rate'):
        return 0, 0.0
    return sum(m.n_draws() for m in mods), float(backbone.drop_path_rate)


@torch.no_grad()
def mc_uncertainty(model, image, num_samples=30, rate=None, generator=None, batch_size=None, radius=1.0, ddof=0, min_conf=None):
    """What `num_samples` stochastic-depth members of the model say about ONE image.

    image: as `occlusion_sensitivity_maps` takes it -- (1,3,H,W) or (3,H,W) fp32 normalised device tensor, or the stem's packed (1,H,W,8)
    bf16.  rate: the stochastic-depth rate (None: the model's drop_path_rate).  generator: a device torch.Generator for the one draw of all
    (n_draws, S) multipliers.  At most `batch_size` members go through the model at a time (None: all at once); a member is the batch-1
    forward under its column of the multipliers, bit for bit, wherever the model's kernels take the same route at both batch sizes
    (DESIGN.md "Predictive uncertainty", Chunks).  radius (heat pixels) and ddof: as `hipops.ensemble_points` / `ensemble_moments`.
    min_conf: members whose peak (decoded score) is below it do not count in `points` (`points_decoded`); None: every finite one counts.
    The model must be in eval mode (RuntimeError) and have a stochastic-depth layer with a non-zero rate (ValueError: an ensemble of
    identical members is not an answer).
    -> dict of device tensors: stack (S,K,h,w) fp32 the members' heat maps; mean, std (K,h,w) fp32; scales (n_draws,S); members (S,K,4)
    float64 = sum, peak, argmax x, argmax y of every member map; mean_summary, std_summary (K,4) the same of mean and std (the ensemble's
    position; the largest std and where it is); points (K,12) `hipops.ENSEMBLE_POINT_COLUMNS` of the members' argmax positions with their
    peaks as conf and the mean map's argmax as centre; with a fusion head also decoded (S,K,2) sub-pixel keypoints, decoded_scores (S,K) and
    points_decoded (K,12) of them (conf: the decoded scores, centre: their mean).  No host synchronisation anywhere."""
    if model.training:
        raise RuntimeError("mc_uncertainty needs eval mode: in training mode batch statistics would couple the members")
    S = int(num_samples)
    if S < 1 + int(ddof):
        raise ValueError(f"mc_uncertainty: num_samples {num_samples} with ddof={ddof}")
    step = S if batch_size is None else int(batch_size)
    if step < 1:
        raise ValueError(f"batch_size {batch_size}")
    n_draws, own = stochastic_depth_draws(model)
    eff = own if rate is None else float(rate)
    if n_draws == 0:
        raise ValueError(f"mc_uncertainty: {type(getattr(model, 'backbone', model)).__name__} has no stochastic-depth layer to sample")
    if not 0.0 < eff < 1.0:
        raise ValueError(f"mc_uncertainty: stochastic-depth rate {eff}: the members would be identical (pass rate= in (0, 1))")
    x = _packed_image(image)
    floor = float('-inf') if min_conf is None else float(min_conf)
    keep = 1.0 - eff
    scales = torch.floor(keep + torch.rand(n_draws, S, device=x.device, generator=generator)) / keep
    fusion = getattr(model, 'head_type', None) == 'fusion'
    stack = decoded = dscore = None
    for first in range(0, S, step):
        n = min(step, S - first)
        with nnops.stochastic_depth(scales=scales[:, first:first + n].contiguous()) as sd:
            out = model(x.expand(n, -1, -1, -1))
        if sd.uses != 1:
            raise ValueError(f"mc_uncertainty: the forward consulted the stochastic-depth context {sd.uses} times, not once")
        hm = out['heatmaps']
        if stack is None:
            stack = torch.empty(S, *hm.shape[1:], dtype=torch.float32, device=x.device)
        stack[first:first + n].copy_(hm)
        if fusion:
            kp, sc = model.head.decode(out, apply_offset=True)
            if decoded is None:
                decoded = torch.empty(S, *kp.shape[1:], dtype=torch.float32, device=x.device)
                dscore = torch.empty(S, sc.shape[1], dtype=torch.float32, device=x.device)
            decoded[first:first + n].copy_(kp)
            dscore[first:first + n].copy_(sc)
    mean, std = hipops.ensemble_moments(stack, ddof)
    members = hipops.heatmap_summary(stack)
    mean_summary, std_summary = hipops.heatmap_summary(mean), hipops.heatmap_summary(std)
    points = hipops.ensemble_points(members[..., 2:4].float().contiguous(), members[..., 1].float().contiguous(),
                                    mean_summary[:, 2:4].contiguous(), floor, radius, ddof)
    res = {'mean': mean, 'std': std, 'stack': stack, 'scales': scales, 'members': members, 'points': points,
           'mean_summary': mean_summary, 'std_summary': std_summary}
    if fusion:
        res['decoded'], res['decoded_scores'] = decoded, dscore
        res['points_decoded'] = hipops.ensemble_points(decoded, dscore, None, floor, radius, ddof)
    return res


class UncertaintyAnalyzer:
    """The reference's class (analysis/advanced_analysis.py), as far as it is ported: the Monte-Carlo uncertainty maps."""

    @staticmethod
    def monte_carlo_dropout_uncertainty(model, image, num_samples=30):
        """The reference's call and return shape: (fig, mean_pred, std_pred) with fig = None (no matplotlib here, as for the other
        analyzers) and numpy (1,K,h,w) float32 arrays, np.mean / np.std (ddof 0) over the members.  Like the reference it puts the model
        into eval mode.  DELIBERATE DIVERGENCE: the members differ by stochastic depth (DropPath at the model's drop_path_rate), not by
        dropout -- the reference's switch turns on nn.Dropout modules whose p is 0 and leaves DropPath off, so its members are identical
        and its std map is zero.  (`mc_uncertainty` keeps everything on the device and gives the per-joint numbers as well.)"""
        model.eval()
        device = next(model.parameters()).device
        res = mc_uncertainty(model, image.to(device), num_samples=num_samples)
        return None, res['mean'][None].cpu().numpy(), res['std'][None].cpu().numpy()
