"""Per-tensor statistics on the device: the numbers behind the reference's analysis/ figures `analyze_gradient_statistics`,
`plot_gradient_flow` and `analyze_weight_distribution` (advanced_analysis.py:157-264, nn_quantitative_viz.py:513-525), without the
figures and without a `.cpu().numpy()` round trip per parameter: the tensors are packed into one flat device buffer, reduced by
pk_tensor_stats in two launches, and 64 bytes per tensor come back in one read.  Like every op here: device tensors only, no fallback.
(A training loop has the flat buffers already: engine.FlatAdamW.tensor_stats reads them in place.)"""
import collections

import numpy as np
import torch

from .. import hipops

DEFAULT_THRESHOLDS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)          # advanced_analysis.py:216


def _pack(named_tensors):
    named = [(n, t) for n, t in named_tensors]
    if not named:
        raise ValueError("tensor_statistics: no tensors")
    for n, t in named:
        hipops._chk(t, torch.float32, n)
        if t.numel() == 0:
            raise ValueError(f"tensor_statistics: {n} is empty")
    dev = named[0][1].device
    offsets, off = [], 0
    for _, t in named:
        offsets.append(off)
        off += -(-t.numel() // 4) * 4          # every tensor starts 16-byte aligned
    flat = torch.zeros(off, dtype=torch.float32, device=dev)
    for (_, t), o in zip(named, offsets):
        flat[o:o + t.numel()].copy_(t.detach().reshape(-1))
    plan = hipops.TensorStatsPlan(offsets, [t.numel() for _, t in named], dev)
    return [n for n, _ in named], flat, plan


def _run(names, flat, plan, tiny):
    recs = hipops.tensor_stats_records(hipops.tensor_stats(plan, flat, tiny=tiny))
    return collections.OrderedDict((n, hipops.derive_tensor_stats(r)) for n, r in zip(names, recs))


def tensor_statistics(named_tensors, tiny=0.0):
    """{name: {mean, std, min, max, norm, abs_mean, abs_max, numel, nonfinite, small}} of an iterable of (name, device fp32 tensor), in
    its order; inf / NaN elements are counted in `nonfinite` and left out of everything else; `small` counts |x| <= tiny."""
    names, flat, plan = _pack(named_tensors)
    return _run(names, flat, plan, tiny)


def gradient_statistics(model):
    """The dictionary of the reference's analyze_gradient_statistics: mean / std / min / max / norm (and the further keys of
    tensor_statistics) of every parameter that has a gradient."""
    return tensor_statistics((n, p.grad) for n, p in model.named_parameters() if p.grad is not None)


def gradient_flow(named_parameters):
    """(names, mean |grad|, max |grad|) per parameter that requires and has a gradient: the bars of the reference's plot_gradient_flow."""
    st = tensor_statistics((n, p.grad) for n, p in named_parameters if p.requires_grad and p.grad is not None)
    return list(st), [v["abs_mean"] for v in st.values()], [v["abs_max"] for v in st.values()]


def _below(level):
    """The largest float32 strictly below `level`: |w| <= it  <=>  |w| < level, the reference's comparison."""
    t = np.float32(level)
    return float(t if float(t) < level else np.nextafter(t, np.float32(0)))


def weight_statistics(model, thresholds=DEFAULT_THRESHOLDS):
    """{"layers": {name: {mean, std, ...}} for every trainable tensor with 'weight' in its name, "sparsity": {threshold: share of all
    those weights with |w| < threshold}}: analyze_weight_distribution's mean +- std per layer and its sparsity curve.  One statistics
    call per threshold (the record holds one small-count); the tensors are packed once."""
    names, flat, plan = _pack((n, p.data) for n, p in model.named_parameters() if "weight" in n and p.requires_grad)
    layers, sparsity = None, collections.OrderedDict()
    for level in thresholds:
        if not (np.isfinite(level) and level > 0):
            raise ValueError(f"weight_statistics: threshold {level} must be finite and > 0")
        st = _run(names, flat, plan, _below(level))
        layers = layers or st
        total = sum(v["numel"] for v in st.values())
        sparsity[level] = sum(v["small"] for v in st.values()) / total
    if layers is None:
        layers = _run(names, flat, plan, 0.0)
    return {"layers": layers, "sparsity": sparsity}


__all__ = ["tensor_statistics", "gradient_statistics", "gradient_flow", "weight_statistics"]
