"""Activation statistics and dead-channel report on the device (rules: DESIGN.md, "Activation statistics").

The reference's `ActivationAnalyzer` (analysis/advanced_analysis.py:15-150) hangs a forward hook on every nn.ReLU, copies each output to
the host and reduces it there with numpy (`np.sort` over the whole tensor for the median).  Here BatchNorm and ReLU sit in the conv's
epilogue in eval mode and the transformer blocks run as fused halves, so there is no nn.ReLU to hook; instead the op layer hands every
activation that exists in memory to a collector (`nnops.observe`), which reduces it where it lies: one bandwidth-bound pass per tapped
tensor for the per-channel records and the 4096-bin table (pk_activation_stats), one more for exact order statistics
(pk_activation_quantiles).  Nothing is read back before the last forward has been queued."""
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib, dispatch, hipops, nnops
from .metrics import _quantile_values

__all__ = ['ActivationAnalyzer', 'ActivationCollector', 'activation_report']


def _check_quantiles(quantiles):
    q = np.asarray(list(quantiles), np.float64).reshape(-1)
    if not 1 <= q.size <= hipops.ACT_MAX_QUANTILES or not bool(np.all((q >= 0.0) & (q <= 1.0))):
        raise ValueError(f"quantiles: expected 1 to {hipops.ACT_MAX_QUANTILES} values in [0, 1], got {q.tolist()}")
    return q


def _exchange_channels(fuse, i):
    """Channels of output i of an exchange unit: what the last BatchNorm of any route into it produces."""
    for route in fuse[str(i)].values():
        bns = [m for m in route.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        if bns:
            return int(bns[-1].num_features)
    return None


class _Layer:
    def __init__(self, kind, relu, c_used):
        self.kind, self.relu, self.c_used = kind, relu, c_used
        self.records = self.hist = self.order = None
        self.batches, self.shape, self.tensors = 0, None, []


class ActivationCollector:
    """What `nnops.observe` calls at every tap.  Layer names are the qualified module names of `model` (a model that runs as its
    8-aligned padded twin is tapped on the twin: same names; `c_used` is the channel count of the REAL module of that name, the twin's
    extra channels lie behind it and are exactly zero).  An exchange output is named after the fuse row that produces it,
    `<...>.fuse_layers.<i>`.  A name met again (a later batch) is accumulated into.  `keep_tensors`: also keep a clone of every tapped
    tensor (tests).  Launches on the stream of the calling branch task; never reads back."""

    def __init__(self, model, quantiles=(0.25, 0.5, 0.75), keep_tensors=False):
        self.q = _check_quantiles(quantiles)
        self.keep = bool(keep_tensors)
        twin = dispatch.padded_twin(model) if next(model.parameters()).is_cuda else None
        run = twin.twin if twin is not None else model
        self.names = {id(m): n for n, m in run.named_modules()}
        self.real = dict(model.named_modules())
        self.layers = OrderedDict()

    def _resolve(self, kind, key, tensor):
        mod, i = key if kind == "exchange" else (key, None)
        name = self.names.get(id(mod))
        if name is None:
            raise RuntimeError(f"activation tap of a {type(mod).__name__} that is not a module of the observed model")
        real = self.real.get(name, mod)
        C = int(tensor.shape[-1])
        if kind == "conv_bn":
            c_used = int(real.num_features)
        elif kind == "window_block":
            c_used = int(getattr(real, "dim", C))
        else:
            c_used, name = _exchange_channels(real, i) or C, f"{name}.{i}"
        return name, min(c_used, C)

    def tap(self, kind, key, tensor, relu):
        name, c_used = self._resolve(kind, key, tensor)
        x = tensor.detach()
        layer = self.layers.get(name)
        if layer is None:
            layer = self.layers[name] = _Layer(kind, bool(relu), c_used)
            layer.records, layer.hist = hipops.activation_stats(x, c_used)
            layer.order = hipops.activation_quantiles(x, layer.hist, self.q, c_used)      # exact while the layer has seen one tensor
        else:
            hipops.activation_stats(x, c_used, layer.records, layer.hist)
            layer.order = None
        layer.batches += 1
        layer.shape = tuple(int(s) for s in x.shape)
        if self.keep:
            layer.tensors.append(x.clone())

    # ---- the one device read
    def fetch(self):
        """-> {name: (records as a structured array, hist (4096,) int64, order (Q,2) float32 or None)}: ONE device-to-host copy."""
        parts, layout = [], []
        for name, L in self.layers.items():
            for t in (L.records, L.hist, L.order):
                if t is not None:
                    parts.append(t.reshape(-1).view(torch.uint8))
            layout.append((name, L.records.numel(), L.hist.numel() * 8, 0 if L.order is None else L.order.numel() * 4))
        if not parts:
            return {}
        flat = torch.cat(parts).cpu().numpy()
        out, pos = {}, 0
        for name, nr, nh, no in layout:
            rec = flat[pos:pos + nr].view(hipops.ACT_RECORD)
            hist = flat[pos + nr:pos + nr + nh].view(np.int64)
            order = flat[pos + nr + nh:pos + nr + nh + no].view(np.float32).reshape(-1, 2) if no else None
            out[name] = (rec, hist, order)
            pos += nr + nh + no
        return out

    def report(self, threshold=1e-6, histogram=False):
        fetched = self.fetch()
        edges = hipops.activation_bin_edges()
        out = OrderedDict()
        for name, L in self.layers.items():
            out[name] = _layer_report(L, *fetched[name], self.q, threshold, edges if histogram else None)
        return out


def _table_order(hist, q):
    """v[lo], v[hi] at the resolution of the table (the smallest value of the bin that holds the rank): what is left of the order
    statistics once a layer has seen several tensors, whose elements no longer exist."""
    edges, cum, n = hipops.activation_bin_edges(), np.cumsum(hist), int(hist.sum())
    order = np.full((len(q), 2), np.nan, np.float32)
    if n:
        pos = q * float(n - 1)
        lo = np.minimum(np.floor(pos).astype(np.int64), n - 1)
        for col, rank in ((0, lo), (1, np.minimum(lo + 1, n - 1))):
            order[:, col] = edges[np.searchsorted(cum, rank, side="right")]
    return order


def _layer_report(L, rec, hist, order, q, threshold, edges):
    n = rec["n"].astype(np.int64)
    fin = n - rec["n_nonfinite"]
    m = int(fin.sum())
    B, C = L.shape[0], L.c_used
    r = OrderedDict(kind=L.kind, relu=L.relu, shape=[B, C] + list(L.shape[1:-1]) if len(L.shape) == 4 else list(L.shape[:-1]) + [C],
                    batches=L.batches, numel=int(n.sum()))
    if m:
        mean = float(rec["sum"].sum()) / m
        lo, hi = float(rec["min"].min()), float(rec["max"].max())
        # E[x^2] - mean^2 cancels to rounding noise of either sign on a constant tensor: min == max says so exactly
        var = 0.0 if lo == hi else max(float(rec["sumsq"].sum()) / m - mean * mean, 0.0)
        r.update(mean=mean, std=float(np.sqrt(var)), min=lo, max=hi)
    else:
        r.update(mean=float("nan"), std=float("nan"), min=float("nan"), max=float("nan"))
    exact = order is not None
    vals = _quantile_values((order if exact else _table_order(hist, q))[None], np.array([m]), q)[0]
    r["quantiles"] = OrderedDict((float(k), float(v)) for k, v in zip(q, vals))
    r["quantiles_exact"] = exact
    total = max(int(n.sum()), 1)
    r["zero_fraction"] = int(rec["n_zero"].sum()) / total
    r["negative_fraction"] = int(rec["n_negative"].sum()) / total
    r["nonfinite"] = int(rec["n_nonfinite"].sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        channel_mean = rec["sum"] / fin
    dead = channel_mean < threshold                               # the reference's rule (a channel without a finite value is not dead: NaN)
    r["channel_mean"] = channel_mean
    r["dead_ratio"] = float(dead.mean())
    r["dead_channels"] = np.flatnonzero(dead).tolist()
    r["always_zero"] = np.flatnonzero(rec["n_zero"] == n).tolist()
    if edges is not None:
        r["histogram"] = {"counts": hist.copy(), "edges": edges}
    return r


def _batches(images, max_batches):
    if torch.is_tensor(images):
        yield images
        return
    for k, batch in enumerate(images):
        if k >= max_batches:
            return
        if isinstance(batch, dict):
            batch = batch["image"] if "image" in batch else batch["img"]
        yield batch


def _device_images(x):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.PoseKernelError("activation_report: images must be device tensors; the activation statistics have no CPU implementation")
    return x


@torch.no_grad()
def activation_report(model, images, quantiles=(0.25, 0.5, 0.75), threshold=1e-6, max_batches=1, histogram=False, collector=None):
    """Statistics of every tapped activation of `model` over up to `max_batches` batches.

    images: a device batch (B,3,H,W), or an iterable of such batches or of dicts with 'image' (the reference's key) or 'img'.  The model
    must be in eval mode (RuntimeError otherwise: the observer is for eval-mode forwards).  -> OrderedDict, layer name -> kind
    ('conv_bn', 'window_block', 'exchange'), relu (whether the tap follows a ReLU), shape (B,C,H,W with the real channel count), batches,
    numel; mean, std (population value, as numpy's), min, max over the finite elements; quantiles {q: value} by numpy's linear rule on the
    two exact order statistics (one tensor per layer; after several batches from the table, `quantiles_exact` False: the smallest value
    of the rank's bin, three mantissa bits); zero_fraction, negative_fraction, nonfinite; channel_mean; dead_ratio = the share of channels
    whose mean over (B,H,W) is < threshold (the reference's rule) with dead_channels, their indices; always_zero = the channels whose
    every element is +-0; with `histogram` the 4096 counts and 4097 edges.  The host is read once, after the last forward."""
    if model.training:
        raise RuntimeError("activation_report needs eval mode: the activation observer is for eval-mode forwards")
    if int(max_batches) < 1:
        raise ValueError(f"max_batches {max_batches}")
    collector = ActivationCollector(model, quantiles) if collector is None else collector
    if torch.is_tensor(images):
        _device_images(images)
    with nnops.observe(collector):
        for x in _batches(images, int(max_batches)):
            model(_device_images(x))
    return collector.report(threshold, histogram)


def activation_report_json(report):
    """`activation_report` with every array as a list and every NaN as None: what `validate.py --activation_report` writes."""
    from .metrics import error_report_json
    return error_report_json({name: {**{k: v for k, v in r.items() if k != "quantiles"},
                                     "quantiles": {repr(k): v for k, v in r["quantiles"].items()}} for name, r in report.items()})


class ActivationAnalyzer:
    """The reference's class (analysis/advanced_analysis.py:15-150), the numbers without the figures."""

    @staticmethod
    def analyze_dead_neurons(model, dataloader, device, threshold=1e-6):
        """The reference's call: puts the model into eval mode, runs the first batch of `dataloader` and returns {layer name: dead_ratio},
        the share of channels whose mean activation is < threshold, over the taps that follow a ReLU plus the window blocks (the
        reference hooks nn.ReLU; see the module docstring for why the names here are those of the BatchNorm / block / fuse row).
        Returns no figure."""
        model.eval()
        first = []
        for batch in dataloader:
            if isinstance(batch, dict):
                batch = batch["image"] if "image" in batch else batch["img"]
            first.append(batch.to(device))
            break
        report = activation_report(model, first, threshold=threshold)
        return {name: r["dead_ratio"] for name, r in report.items() if r["relu"] or r["kind"] == "window_block"}

    @staticmethod
    def analyze_activation_distribution(activations):
        """The numbers behind the reference's four panels for one tensor: mean, std, min, max, median, zero_percent (its "Dead neurons"
        line: elements equal to 0), negative_percent, and channel_means.  activations: a device (B,C,H,W) fp32 or bf16 tensor.  The
        (B,C,H,W) bf16 view a backbone returns of its internal NHWC map is read where it lies, without a copy.  fp32 input is rounded to
        bf16 first (pk_nchw_f32_to_nhwc_bf16), so these are the values the network computes with, not the fp32 ones.  One device read."""
        x = activations
        if not (torch.is_tensor(x) and x.is_cuda):
            raise _lib.PoseKernelError("analyze_activation_distribution: expected a device tensor; the statistics have no CPU implementation")
        if x.dim() != 4:
            raise ValueError(f"analyze_activation_distribution: expected (B,C,H,W), got {tuple(x.shape)}")
        C = int(x.shape[1])
        if x.dtype == torch.bfloat16:
            Cp = -(-C // 8) * 8
            t = x.permute(0, 2, 3, 1)
            t = t.contiguous() if Cp == C else torch.nn.functional.pad(t, (0, Cp - C)).contiguous()
        else:
            t = nnops.to_features(x.float(), cpad=-(-C // 8) * 8)
        L = _Layer("tensor", False, C)
        q = np.array([0.5])
        L.records, L.hist = hipops.activation_stats(t, C)
        L.order = hipops.activation_quantiles(t, L.hist, q, C)
        L.batches, L.shape = 1, tuple(int(s) for s in t.shape)
        flat = torch.cat([a.reshape(-1).view(torch.uint8) for a in (L.records, L.hist, L.order)]).cpu().numpy()
        nr, nh = L.records.numel(), L.hist.numel() * 8
        r = _layer_report(L, flat[:nr].view(hipops.ACT_RECORD), flat[nr:nr + nh].view(np.int64),
                          flat[nr + nh:].view(np.float32).reshape(-1, 2), q, 1e-6, None)
        return {"mean": r["mean"], "std": r["std"], "min": r["min"], "max": r["max"], "median": r["quantiles"][0.5],
                "zero_percent": 100.0 * r["zero_fraction"], "negative_percent": 100.0 * r["negative_fraction"],
                "channel_means": r["channel_mean"]}
