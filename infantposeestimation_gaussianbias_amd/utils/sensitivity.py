"""Occlusion sensitivity on the device (rules: DESIGN.md, "Occlusion sensitivity").

The reference's `SensitivityAnalyzer.occlusion_sensitivity` (analysis/advanced_analysis.py:387-427) blanks one patch of the crop at a time,
runs a batch-1 forward and reads one heat-map sum back to the host -- 660 forwards and 661 synchronisations at 256 x 192 with patch 16 and
stride 8, for one joint.  In eval mode every sample of a batch is independent of the others and bit-reproducible, so here the occluded
copies are made in the stem's packed layout by one kernel per chunk (pk_occlude_batch), go through the model `batch_size` at a time, every
output map is reduced to its score by one kernel per chunk (pk_heatmap_summary), and one kernel paints the reference's map of EVERY joint
from the score table (pk_occlusion_paint).  Nothing is read back in between.

Gradient attribution (rules: DESIGN.md, "Gradient attribution").  The reference's `SensitivityAnalyzer.compute_input_sensitivity`
(analysis/advanced_analysis.py:317-342) and `GradCAMVisualizer.generate_cam` (analysis/nn_quantitative_viz.py:358-415) run one batch-1
forward and backward per joint.  The same independence of the samples gives the maps of ALL joints from one batched forward and one batched
backward: copy i of the crop is seeded with joint i's map (`attribution_maps`).  The stem's data gradient (pk_stem_dgrad), the reduction of
the packed gradient (pk_saliency_reduce, pk_nhwc_bf16_to_nchw_f32) and Grad-CAM (pk_gradcam) are kernels; nothing is read back."""
import numpy as np
import torch

from .. import _lib, dispatch, hipops, nnops
from .activations import ActivationCollector

__all__ = ['GradCAMVisualizer', 'GradientCollector', 'SensitivityAnalyzer', 'attribution_maps', 'occlusion_sensitivity_maps']


def _packed_image(image, who="occlusion_sensitivity_maps", what="sweep", single=True):
    """(1,3,H,W) or (3,H,W) fp32 normalised, or the packed (1,H,W,8) / (H,W,8) bf16 -> (1,H,W,8) bf16, packed once.  `single` False
    (utils/feature_maps.py): a batch of either is taken as well."""
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise TypeError(f"{who}: image must be a device tensor (the {what} has no CPU implementation)")
    if image.dtype == torch.bfloat16 and image.shape[-1] == 8 and image.dim() in (3, 4):
        image = image[None] if image.dim() == 3 else image
    elif image.dim() in (3, 4) and image.shape[-3] == 3:
        image = image[None] if image.dim() == 3 else image
    else:
        raise ValueError(f"{who}: image {tuple(image.shape)} is neither (1,3,H,W) / (3,H,W) nor the packed (1,H,W,8) bf16")
    if single and image.shape[0] != 1:
        raise ValueError(f"{who}: one image at a time, got a batch of {image.shape[0]}")
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


# ================================================================================================ gradient attribution
class GradientCollector(ActivationCollector):
    """What `nnops.observe` calls at every tap, for gradients: of the layers named in `wanted` it keeps the tapped tensor and hangs a
    tensor hook on it that keeps its gradient.  Layer names and `c_used` are `ActivationCollector`'s (qualified module names, exchange
    outputs `<...>.fuse_layers.<i>`, a padded twin tapped on the twin with the real module's channel count).  `seen` lists every name
    tapped, in order.  The forward must run with grad enabled.  Nothing is launched here and nothing read back."""

    def __init__(self, model, wanted=()):
        super().__init__(model)
        self.wanted = tuple(wanted)
        self.seen = []
        self.taps = {}                                            # name -> [activation, c_used, gradient or None, event or None]

    def tap(self, kind, key, tensor, relu):
        name, c_used = self._resolve(kind, key, tensor)
        self.seen.append(name)
        if name not in self.wanted:
            return
        if not tensor.requires_grad:
            raise RuntimeError(f"gradient tap of {name}: the tensor does not require grad (run the forward with grad enabled on an input or "
                               "parameters that require it)")
        entry = self.taps[name] = [tensor, c_used, None, None]

        def keep(grad):
            # runs on the stream the tapped tensor was produced on (a branch's side stream perhaps): the reader waits for this event
            entry[2], entry[3] = grad, torch.cuda.Event()
            entry[3].record()

        tensor.register_hook(keep)

    def pairs(self):
        """-> {name: (activation, gradient, c_used)} once backward has run, safe to read on the current stream."""
        out, cur = {}, torch.cuda.current_stream()
        for name in self.wanted:
            if name not in self.taps or self.taps[name][2] is None:
                raise RuntimeError(f"gradient tap of {name}: no gradient arrived (the layer does not lie between the input and the score)")
            a, c_used, g, ev = self.taps[name]
            cur.wait_event(ev)
            g.record_stream(cur)
            out[name] = (a.detach(), g, c_used)
        return out


def _default_cam_layer(collector):
    """The backbone's output: output 0 of the last exchange unit, named after its fuse row."""
    fuses = [n for n in collector.names.values() if n.endswith("fuse_layers")]
    if not fuses:
        raise ValueError("attribution: the model has no exchange unit, name the target layer")
    return fuses[-1] + ".0"


def _target_layers(collector, target_layers):
    if target_layers is None:
        return (_default_cam_layer(collector),)
    if isinstance(target_layers, str):
        return (target_layers,)
    return tuple(target_layers)


def _refuse_for_attribution(model, who):
    """What can be said without touching the device: eval mode, and no optimiser's gradient sinks on the real parameters."""
    if model.training:
        raise RuntimeError(f"{who} needs eval mode: in training mode batch statistics would couple the copies")
    if any(getattr(p, "_pk_grad_sink", None) is not None for p in model.parameters()):
        raise _lib.PoseKernelError(f"{who}: the model's parameters carry an optimiser's gradient sinks (a Trainer's model): the attribution backward "
                                   "would store into them.  Attribution during training is not supported; use a model without a Trainer")


class _attribution_scope:
    """Keeps an attribution backward from leaving anything behind: a padded twin's gradients are not scattered into the real parameters
    (its private gradient buffer may be written), its parameters' `used` marks are put back, and the postponed slab reductions of this
    backward are dropped instead of being left for a later step."""

    def __init__(self, model):
        self.tw = dispatch.padded_twin(model) if next(model.parameters()).is_cuda else None

    def __enter__(self):
        if self.tw is not None:
            self.used = [(p, p._pk_used) for p in self.tw.tp.values()]
        return self

    def backward(self, outputs, inputs, seed):
        if self.tw is not None:
            self.tw._pending = False                              # the extraction queued by the forward finds nothing to do
        return torch.autograd.grad([outputs], [inputs], [seed])[0]

    def __exit__(self, *exc):
        nnops.discard_deferred()
        if self.tw is not None:
            self.tw._pending = False
            for p, u in self.used:
                p._pk_used = u


def _heatmaps_of(out):
    return out['heatmaps'] if isinstance(out, dict) else out


def _attribution_pass(model, copies, seed_of, layers):
    """One forward with grad under a gradient collector and one backward from `seed_of(heatmaps)`.
    -> (heatmaps detached, packed input gradient, {layer: (A, G, c_used)}).  An unknown layer is a ValueError that lists the tapped names."""
    collector = GradientCollector(model, layers)
    with _attribution_scope(model) as scope, torch.enable_grad():
        with nnops.observe(collector):
            hm = _heatmaps_of(model(copies))
        unknown = [n for n in layers if n not in collector.taps]
        if unknown:
            raise ValueError(f"attribution: no tapped layer named {', '.join(map(repr, unknown))}; the tapped layers are: "
                             f"{', '.join(dict.fromkeys(collector.seen))}")
        g = scope.backward(hm, copies, seed_of(hm))
        pairs = collector.pairs()
    return hm.detach(), g, pairs


def attribution_maps(model, image, joints=None, target_layers=None, batch_size=32):
    """Input saliency and Grad-CAM of the given joints (None: all K) from one batched forward and one batched backward per chunk.

    image: as in `occlusion_sensitivity_maps`: (1,3,H,W) or (3,H,W) fp32 normalised device tensor, or the stem's packed (1,H,W,8) bf16.
    It is not touched: neither its `requires_grad` nor its `.grad` (the reference sets `requires_grad` on the caller's tensor).
    target_layers: None = the backbone's output (output 0 of the last exchange unit); a layer name or a list of names as
    `ActivationCollector` gives them; () = saliency only.  An unknown name is a ValueError that lists the tapped names.
    The model must be in eval mode (RuntimeError otherwise: batch statistics would couple the copies) and must not carry an optimiser's
    gradient sinks (a Trainer's model: refused).  Per chunk of n <= batch_size joints: n copies of the packed crop that require grad, one
    forward under the gradient collector, the score sum_i heatmaps[i, joints[i]].sum(), one backward to the copies; pk_saliency_reduce
    and pk_nhwc_bf16_to_nchw_f32 on the packed gradient, pk_gradcam per layer, pk_heatmap_summary of the forward.  The weight gradients
    of that backward are computed and discarded; parameter `.grad` fields stay as they were.  No read-back, no synchronisation.
    -> dict, everything on the device: saliency (J,H,W) fp32 = max over the colour channels of |d score / d image|; grad (J,3,H,W) fp32;
    cams {layer: (J,h,w) fp32 in [0,1]}; cam_weights {layer: (J,c_used) fp32}; cam_range {layer: (J,2) float64: min and max of the
    un-normalised map}; base (J,4) float64: sum, max, argmax x, argmax y of each joint's heat map; layers: the resolved names."""
    _refuse_for_attribution(model, "attribution_maps")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size {batch_size}")
    x = _packed_image(image.detach() if isinstance(image, torch.Tensor) else image, "attribution_maps", "attribution")
    if joints is None:
        K = getattr(model, "num_keypoints", None)
        if K is None:
            raise ValueError("attribution_maps: joints=None needs a model with `num_keypoints`; name the joints")
        joints = range(int(K))
    joints = [int(j) for j in joints]
    if not joints:
        raise ValueError("attribution_maps: no joints")
    layers = _target_layers(ActivationCollector(model), target_layers)
    dev, J, step = x.device, len(joints), min(int(batch_size), len(joints))
    H, W = int(x.shape[1]), int(x.shape[2])
    joints_t = torch.tensor(joints, dtype=torch.int64, device=dev)
    rows = torch.arange(step, device=dev)
    sal, grads, base = [], [], []
    cams, cam_w, cam_r = ({n: [] for n in layers} for _ in range(3))
    for first in range(0, J, step):
        n = min(step, J - first)
        jt = joints_t[first:first + n]
        copies = x.repeat(n, 1, 1, 1).requires_grad_(True)        # always a new tensor: the caller's is never marked

        def seed_of(hm):
            K = int(hm.shape[1])
            if min(joints) < 0 or max(joints) >= K:
                raise ValueError(f"attribution_maps: joints {joints} outside 0 .. {K - 1}")
            seed = torch.zeros(n, K, dtype=hm.dtype, device=dev)
            seed[rows[:n], jt] = 1.0                              # d score / d heatmaps: ones over map (i, joints[i]), zeros elsewhere
            return seed[:, :, None, None].expand_as(hm)

        hm, g, pairs = _attribution_pass(model, copies, seed_of, layers)
        sal.append(hipops.saliency_reduce(g, 3))
        grads.append(hipops.packed_grad_to_nchw(g, 3))
        base.append(hipops.heatmap_summary(hm)[rows[:n], jt])
        for name, (A, G, c_used) in pairs.items():
            cam, wts, rng = hipops.grad_cam(A, G, c_used)
            cams[name].append(cam), cam_w[name].append(wts), cam_r[name].append(rng)

    def cat(parts):
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    return {'saliency': cat(sal), 'grad': cat(grads), 'cams': {n: cat(v) for n, v in cams.items()},
            'cam_weights': {n: cat(v) for n, v in cam_w.items()}, 'cam_range': {n: cat(v) for n, v in cam_r.items()}, 'base': cat(base),
            'layers': list(layers)}


class GradCAMVisualizer:
    """The reference's class (analysis/nn_quantitative_viz.py:358-415), the map without the figure.  `target_layer`: a tapped layer's
    name (None: the backbone's output); the reference hooks a module, here the op layer hands the activation and its gradient over."""

    def __init__(self, model, target_layer=None):
        self.model, self.target_layer = model, target_layer

    def generate_cam(self, input_image, target_class=None):
        """The reference's call: a (1,1,h,w) fp32 device tensor in [0,1].  Puts the model into eval mode, as the reference does.
        target_class: a joint index.  None scores the SUM OF ALL joints' maps -- a deviation: the reference indexes `output[0,
        output.argmax(dim=1)]`, a (1,h,w) tensor of channel indices used as an index into the K maps, which is ill-defined for heat maps
        (it picks whole maps by the per-pixel winning channel, many times over)."""
        self.model.eval()
        image = input_image.to(next(self.model.parameters()).device)
        if target_class is not None:
            out = attribution_maps(self.model, image, joints=[int(target_class)], target_layers=self.target_layer, batch_size=1)
            return out['cams'][out['layers'][0]][:, None]
        _refuse_for_attribution(self.model, "generate_cam")
        x = _packed_image(image.detach(), "generate_cam", "attribution")
        layers = _target_layers(ActivationCollector(self.model), self.target_layer)[:1]
        _, _, pairs = _attribution_pass(self.model, x.clone().requires_grad_(True), torch.ones_like, layers)
        A, G, c_used = pairs[layers[0]]
        return hipops.grad_cam(A, G, c_used)[0][:, None]


class SensitivityAnalyzer:
    """The reference's class (analysis/advanced_analysis.py), the numbers without the figures: the occlusion map and the input saliency."""

    @staticmethod
    def compute_input_sensitivity(model, input_image, target_keypoint):
        """The reference's call: a numpy (H,W) fp32 map, max over the colour channels of |d heatmaps[0, target_keypoint].sum() / d image|.
        Like the reference it puts the model into eval mode; unlike it, it leaves `input_image.requires_grad` alone.
        (`attribution_maps` gives all joints, and Grad-CAM, for one batched pass and keeps them on the device.)"""
        model.eval()
        device = next(model.parameters()).device
        out = attribution_maps(model, input_image.to(device), joints=[int(target_keypoint)], target_layers=(), batch_size=1)
        return out['saliency'][0].cpu().numpy()

    @staticmethod
    def occlusion_sensitivity(model, image, target_keypoint, patch_size=16, stride=8):
        """The reference's call: a numpy (H,W) float64 map of joint `target_keypoint`, the drop of that joint's heat-map sum under every
        patch.  Like the reference it puts the model into eval mode.  (`occlusion_sensitivity_maps` gives all joints for the same cost and
        keeps them on the device.)"""
        model.eval()
        device = next(model.parameters()).device
        maps = occlusion_sensitivity_maps(model, image.to(device), patch_size, stride)['maps']
        return maps[target_keypoint].cpu().numpy().astype(np.float64, copy=False)
