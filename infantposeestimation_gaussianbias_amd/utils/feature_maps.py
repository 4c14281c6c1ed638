"""Feature-map sheets and heat-map quality on the device (rules: DESIGN.md, "Feature sheets and heat-map quality").

The reference's `FeatureVisualizer` (analysis/nn_quantitative_viz.py:255-324) copies a layer's output to the host, normalises every
channel with numpy and hands the tiles to matplotlib; its heat-map comparison does the same with three `imshow` panels per joint and
gives no number.  Here the tapped tensor stays where it lies: the wanted channels of the NHWC map become planes (pk_gather_planes), one
kernel pair scales every tile to its own range and paints the finished uint8 sheet (pk_plane_sheet), and every (prediction, target) pair of
maps gets a record of sums, peaks, co-moments and half-maximum overlap (pk_heatmap_quality) from which the quality numbers are derived.
Nothing is copied to the host before the caller asks for it.  `FeatureVisualizer.visualize_feature_tsne` has no counterpart here."""
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib, hipops, nnops
from .activations import ActivationCollector
from .sensitivity import _packed_image
from .visualization import _device, _table, colour_ramp

__all__ = ['FeatureCollector', 'FeatureVisualizer', 'HeatmapQualityAccumulator', 'feature_sheet', 'heatmap_quality', 'heatmap_quality_sheet',
           'quality_report_json']

SHEET_SIDE = 2048                                                 # zoom=None: the largest zoom that keeps the sheet within this, per side
_BACKGROUND = (255, 255, 255)


class FeatureCollector(ActivationCollector):
    """What `nnops.observe` calls at every tap, for feature maps: of the layers named in `wanted` it keeps a detached reference to the
    tapped tensor with its `c_used`, and reduces nothing.  Layer names and `c_used` are `ActivationCollector`'s (qualified module names,
    exchange outputs `<...>.fuse_layers.<i>`, a padded twin tapped on the twin with the real module's channel count).  `seen` lists every
    name tapped, in order.  Nothing is launched here and nothing read back."""

    def __init__(self, model, wanted):
        super().__init__(model)
        self.wanted = (wanted,) if isinstance(wanted, str) else tuple(wanted)
        self.seen = []
        self.features = {}                                        # name -> (tensor, c_used, event)

    def tap(self, kind, key, tensor, relu):
        name, c_used = self._resolve(kind, key, tensor)
        self.seen.append(name)
        if name in self.wanted:
            # recorded on the stream the tensor was produced on (a branch's side stream perhaps): the reader waits for this event
            event = torch.cuda.Event()
            event.record()
            self.features[name] = (tensor.detach(), c_used, event)

    def feature(self, name):
        """-> (tensor, c_used) of a wanted layer, safe to read on the current stream.  An unknown name is a ValueError that lists the
        tapped names."""
        if name not in self.features:
            raise ValueError(f"feature maps: no tapped layer named {name!r}; the tapped layers are: {', '.join(dict.fromkeys(self.seen))}")
        x, c_used, event = self.features[name]
        cur = torch.cuda.current_stream()
        cur.wait_event(event)
        x.record_stream(cur)
        return x, c_used


def _auto_zoom(T, h, w, cols, pad):
    rows = -(-T // cols)
    fit = lambda n, size: (SHEET_SIDE - pad - n * pad) // (n * size)      # noqa: E731
    return int(max(1, min(fit(rows, h), fit(cols, w), _lib.CONSTANTS["PK_PANEL_MAX_ZOOM"])))


def _channel_list(channels, c_used, who):
    if isinstance(channels, (int, np.integer)):
        if int(channels) < 1:
            raise ValueError(f"{who}: channels={channels}: at least one")
        return list(range(min(int(channels), c_used)))             # the reference's num_samples = min(num_samples, num_channels)
    chans = [int(c) for c in channels]
    bad = [c for c in chans if not 0 <= c < c_used]
    if not chans or bad:
        raise ValueError(f"{who}: channels {chans if not chans else bad} outside 0 .. {c_used - 1} (the layer's real channels)")
    return chans


def _map_sheet(x, c_used, channels, sample, cols, zoom, pad, ramp, who):
    """Sheet of channels of sample `sample` of a tapped (B,H,W,C) bf16 map."""
    if x.dim() != 4:
        raise ValueError(f"{who}: the tap is not a (B,H,W,C) map: its shape is {tuple(x.shape)}")
    B, H, W, _ = (int(s) for s in x.shape)
    if not 0 <= int(sample) < B:
        raise ValueError(f"{who}: sample {sample} of a batch of {B}")
    chans = _channel_list(channels, c_used, who)
    planes = hipops.gather_planes(x, _table("channels", chans, np.int32, x.device), int(sample), c_used)
    sheet, ranges = _tiles_sheet(planes, len(chans), cols, zoom, pad, ramp)
    return sheet, ranges, chans


def _tiles_sheet(planes, n, cols, zoom, pad, ramp):
    """One tile per plane, all through one ramp."""
    _, h, w = (int(s) for s in planes.shape)
    zoom = _auto_zoom(n, h, w, int(cols), int(pad)) if zoom is None else int(zoom)
    tiles = np.stack([np.arange(n), np.full(n, -1), np.zeros(n, np.int64)], axis=1)
    return hipops.plane_sheet(planes, _table("tiles", tiles, np.int32, planes.device), _table("ramp", colour_ramp(ramp), np.uint8, planes.device),
                              cols=int(cols), zoom=zoom, pad=int(pad), background=_BACKGROUND)


def feature_sheet(model, image, layer, channels=16, sample=0, cols=4, zoom=None, pad=2, ramp='sequential'):
    """A layer's channels as one sheet of colour-mapped tiles, each scaled to its own range (the reference's
    `(f - f.min()) / (f.max() - f.min() + 1e-8)`), `cols` tiles per row, every element zoom x zoom pixels.

    image: as `attribution_maps` takes it -- (1,3,H,W) or (3,H,W) fp32 normalised device tensor or the stem's packed (1,H,W,8) bf16 -- or a
    batch of those, of which `sample` is shown.  It is not touched.  layer: a name as `ActivationCollector` gives them; an unknown name is a
    ValueError that lists the tapped names.  channels: an int for the first n channels, capped at the layer's real channel count (the
    reference's rule), or an explicit list (ValueError outside the real channels).  zoom None: the largest zoom that keeps the sheet within
    2048 pixels per side, at least 1.  ramp: a name `colour_ramp` knows.  One eval-mode forward under `nnops.observe`, without grad; the
    model's mode is restored afterwards.  A tap that is not a 4-D (B,H,W,C) map raises, naming its shape.  No read-back.
    -> (sheet (SH,SW,3) uint8 BGR device tensor, ranges (n,2) fp32 device tensor: minimum and maximum of each tile, the channel list)."""
    x = _packed_image(image.detach() if isinstance(image, torch.Tensor) else image, "feature_sheet", "feature sheet", single=False)
    collector = FeatureCollector(model, (layer,))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), nnops.observe(collector):
            model(x)
    finally:
        model.train(was_training)
    feat, c_used = collector.feature(layer)
    return _map_sheet(feat, c_used, channels, sample, cols, zoom, pad, ramp, f"feature_sheet({layer})")


# ================================================================================================ heat-map quality
def _derive(rec, hw):
    """Quality numbers from (..., 16) float64 records (torch, on whatever device they lie): a dict of (...) tensors."""
    nan = torch.full_like(rec[..., 0], float("nan"))
    n = float(hw) - rec[..., 15]
    den = rec[..., 11] * rec[..., 12]
    dx, dy = rec[..., 5] - rec[..., 8], rec[..., 6] - rec[..., 9]
    return OrderedDict(
        mse=torch.where(n > 0, rec[..., 2] / n, nan),
        max_abs_diff=rec[..., 3],
        peak_pred=torch.stack([rec[..., 5], rec[..., 6], rec[..., 4]], dim=-1),
        peak_gt=torch.stack([rec[..., 8], rec[..., 9], rec[..., 7]], dim=-1),
        peak_distance=torch.sqrt(dx * dx + dy * dy),
        correlation=torch.where(den > 0, rec[..., 10] / torch.sqrt(den), nan),
        iou_half_max=torch.where(rec[..., 14] > 0, rec[..., 13] / rec[..., 14], nan),
        mass_ratio=torch.where(rec[..., 1] != 0, rec[..., 0] / rec[..., 1], nan),
        n_nonfinite=rec[..., 15])


def _device_maps(x, name, who):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise _lib.PoseKernelError(f"{who}: {name}: expected a CUDA(HIP) tensor; the heat-map quality has no CPU implementation")
    return x.detach().float()


def heatmap_quality(pred, gt, weight=None):
    """How good predicted heat maps are as maps.  pred, gt: (..., h, w) device tensors (bf16 is widened); weight: (...) or None.
    -> dict of per-map device tensors, float64 unless said otherwise: mse = sum (p - g)^2 / n; max_abs_diff; peak_pred, peak_gt (..., 3) =
    x, y, value of the maximum (the first of equal maxima); peak_distance between the two, in heat-map pixels; correlation = Pearson's r
    of the two maps (NaN when either is constant); iou_half_max = intersection over union of the regions above half of each map's own
    peak (NaN when the union is empty: a peak that is <= 0 or missing); mass_ratio = sum p / sum g (NaN when sum g is 0);
    n_nonfinite = elements left out because p or g is not finite (n = the others); valid = weight > 0 (all True without a weight), bool;
    records: the (..., 16) float64 rows of pk_heatmap_quality.  One launch and plumbing; no read-back."""
    p, g = _device_maps(pred, "pred", "heatmap_quality"), _device_maps(gt, "gt", "heatmap_quality")
    rec = hipops.heatmap_quality(p, g)
    out = _derive(rec, int(p.shape[-2]) * int(p.shape[-1]))
    lead = tuple(rec.shape[:-1])
    if weight is None:
        out["valid"] = torch.ones(lead, dtype=torch.bool, device=rec.device)
    else:
        if tuple(weight.shape) != lead:
            raise ValueError(f"heatmap_quality: weight {tuple(weight.shape)} for maps {lead}")
        out["valid"] = weight.to(rec.device) > 0
    out["records"] = rec
    return out


_MEANS = ("mse", "max_abs_diff", "peak_distance", "correlation", "iou_half_max", "mass_ratio")


class HeatmapQualityAccumulator:
    """Heat-map quality over a validation set.  `update` stores the records of a batch on the device and never reads back; `compute`
    makes ONE device-to-host copy and takes per-joint and pooled means over the samples whose weight is > 0."""

    def __init__(self, num_keypoints):
        self.K = int(num_keypoints)
        self.records, self.weights, self.hw = [], [], None

    def update(self, pred, gt, weight=None):
        """pred, gt (B,K,h,w) device tensors; weight (B,K) or (B,K,1) or None (every joint counts)."""
        p, g = _device_maps(pred, "pred", "HeatmapQualityAccumulator"), _device_maps(gt, "gt", "HeatmapQualityAccumulator")
        if p.dim() != 4 or p.shape[1] != self.K or tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"HeatmapQualityAccumulator: pred {tuple(p.shape)} and gt {tuple(g.shape)} must both be (B, {self.K}, h, w)")
        hw = (int(p.shape[2]), int(p.shape[3]))
        if self.hw not in (None, hw):
            raise ValueError(f"HeatmapQualityAccumulator: maps of {hw} after maps of {self.hw}")
        self.hw = hw
        B = int(p.shape[0])
        if weight is None:
            w = torch.ones(B, self.K, dtype=torch.float64, device=p.device)
        else:
            w = weight.to(p.device).reshape(B, -1).double()
            if tuple(w.shape) != (B, self.K):
                raise ValueError(f"HeatmapQualityAccumulator: weight {tuple(weight.shape)} for {B} x {self.K} maps")
        self.records.append(hipops.heatmap_quality(p, g))
        self.weights.append(w)

    def compute(self):
        """-> dict: n_samples; map_size (h, w); joints: per joint n (samples with weight > 0) and the means of mse, max_abs_diff,
        peak_distance, correlation, iou_half_max, mass_ratio over them (a NaN entry -- a constant map's correlation -- is left out of its
        mean; NaN when nothing is left) plus n_nonfinite, their sum; pooled: the same over every counted (sample, joint);
        records (N,K,16) float64 and weight (N,K) as numpy arrays."""
        if not self.records:
            raise RuntimeError("HeatmapQualityAccumulator: compute() before any update()")
        N = sum(int(r.shape[0]) for r in self.records)
        flat = torch.cat([torch.cat(self.records).reshape(-1), torch.cat(self.weights).reshape(-1)]).cpu()        # the one device read
        n_rec = N * self.K * hipops.QUALITY_COLS
        rec, weight = flat[:n_rec].reshape(N, self.K, hipops.QUALITY_COLS), flat[n_rec:].reshape(N, self.K)
        q = {k: v.numpy() for k, v in _derive(rec, self.hw[0] * self.hw[1]).items()}
        valid = weight.numpy() > 0

        def means(mask):
            out = OrderedDict(n=int(mask.sum()))
            for k in _MEANS:
                v = q[k][mask]
                v = v[~np.isnan(v)]
                out[k] = float(v.mean()) if v.size else float("nan")
            out["n_nonfinite"] = int(q["n_nonfinite"][mask].sum())
            return out

        only = lambda k: valid & (np.arange(self.K) == k)                        # noqa: E731
        joints = [OrderedDict(joint=k, **means(only(k))) for k in range(self.K)]
        return OrderedDict(n_samples=N, map_size=list(self.hw), joints=joints, pooled=means(valid), records=rec.numpy(), weight=weight.numpy())


def quality_report_json(report):
    """`HeatmapQualityAccumulator.compute()` without the raw records, every NaN as None: what `validate.py --heatmap_quality` writes."""
    from .metrics import error_report_json
    return error_report_json({k: v for k, v in report.items() if k not in ("records", "weight")})


def heatmap_quality_sheet(pred, gt, zoom=None, pad=2):
    """The reference's three-column figure as one sheet: row j = target ('hot'), prediction ('hot'), |prediction - target| ('diverging'),
    each panel scaled to its own range, as `imshow` does.  pred, gt (K,h,w) device tensors.  zoom None: the largest zoom that keeps the
    sheet within 2048 pixels per side, at least 1.  -> (sheet (SH,SW,3) uint8 BGR device tensor, ranges (K,3,2) fp32 device tensor:
    minimum and maximum of every panel, to label them).  One pair of launches, no read-back."""
    p, g = _device_maps(pred, "pred", "heatmap_quality_sheet"), _device_maps(gt, "gt", "heatmap_quality_sheet")
    if p.dim() != 3 or tuple(p.shape) != tuple(g.shape) or p.shape[0] < 1:
        raise ValueError(f"heatmap_quality_sheet: pred {tuple(p.shape)} and gt {tuple(g.shape)} must both be (K, h, w)")
    K, h, w = (int(s) for s in p.shape)
    if 3 * K > hipops.PANEL_MAX_TILES:
        raise ValueError(f"heatmap_quality_sheet: {K} joints ({hipops.PANEL_MAX_TILES // 3} at most on one sheet)")
    zoom = _auto_zoom(3 * K, h, w, 3, int(pad)) if zoom is None else int(zoom)
    j = np.arange(K)
    tiles = np.stack([np.stack([j, np.full(K, -1), np.zeros(K, np.int64)], 1),            # a = target planes then prediction planes
                      np.stack([K + j, np.full(K, -1), np.zeros(K, np.int64)], 1),
                      np.stack([K + j, j, np.ones(K, np.int64)], 1)], axis=1).reshape(3 * K, 3)
    luts = np.stack([colour_ramp('hot'), colour_ramp('diverging')])
    g = g.contiguous()
    sheet, ranges = hipops.plane_sheet(torch.cat([g, p]), _table("tiles", tiles, np.int32, p.device), _table("ramps", luts, np.uint8, p.device),
                                       b=g, cols=3, zoom=zoom, pad=int(pad), background=_BACKGROUND)
    return sheet, ranges.view(K, 3, 2)


class FeatureVisualizer:
    """The reference's class (analysis/nn_quantitative_viz.py:255-324), the images without the matplotlib figures: both calls return the
    sheet as a (SH,SW,3) uint8 BGR array of the kind that came in (numpy for numpy, a device tensor for a device tensor).  Titles and axes
    are not drawn; `feature_sheet` and `heatmap_quality_sheet` also return the ranges to label the tiles with."""

    @staticmethod
    def visualize_feature_maps(features, layer_name, num_samples=16):
        """The reference's call: the first min(num_samples, C) channels of sample 0, four tiles per row, each scaled to its own range.
        features: a (B,C,H,W) fp32 tensor or numpy array, or a tapped (B,H,W,C) bf16 device tensor (C a multiple of 8).  Anything that is
        not 4-D returns None, as the reference does.  `layer_name` titled the reference's figure and is not drawn."""
        if len(features.shape) != 4:
            return None
        if isinstance(features, torch.Tensor) and features.dtype == torch.bfloat16:
            if not features.is_cuda:
                raise _lib.PoseKernelError("visualize_feature_maps: expected a device tensor; the feature sheet has no CPU implementation")
            return _map_sheet(features.detach(), int(features.shape[-1]), int(num_samples), 0, 4, None, 2, 'sequential',
                              f"visualize_feature_maps({layer_name})")[0]
        as_numpy = not isinstance(features, torch.Tensor)
        if as_numpy:
            x = torch.from_numpy(np.array(np.asarray(features)[0], np.float32)).to(_device())
        elif not features.is_cuda:
            raise _lib.PoseKernelError("visualize_feature_maps: expected a device tensor or a numpy array; the feature sheet has no CPU implementation")
        else:
            x = features.detach()[0].float()
        if int(num_samples) < 1:
            raise ValueError(f"visualize_feature_maps: num_samples={num_samples}: at least one")
        n = min(int(num_samples), int(x.shape[0]))
        sheet = _tiles_sheet(x[:n].contiguous(), n, 4, None, 2, 'sequential')[0]
        return sheet.cpu().numpy() if as_numpy else sheet

    @staticmethod
    def visualize_heatmap_quality(pred_heatmap, gt_heatmap, joint_names):
        """The reference's call: pred_heatmap, gt_heatmap (K,h,w), numpy or device tensors; row j shows target, prediction and absolute
        difference of joint j.  `joint_names` titled the reference's panels and is only checked for its length here."""
        if len(joint_names) != int(pred_heatmap.shape[0]):
            raise ValueError(f"visualize_heatmap_quality: {len(joint_names)} joint names for {int(pred_heatmap.shape[0])} maps")
        as_numpy = not isinstance(pred_heatmap, torch.Tensor)
        up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, np.float32)).to(_device())     # noqa: E731
        sheet = heatmap_quality_sheet(up(pred_heatmap), up(gt_heatmap))[0]
        return sheet.cpu().numpy() if as_numpy else sheet
