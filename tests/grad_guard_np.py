"""numpy float64 restatement of the guarded optimiser step (csrc/pk_optim.hip: pk_grad_sumsq -> pk_grad_guard_finalize ->
pk_adamw_step_guarded), for the tests and scripts/bench_grad_guard.py.  Test infrastructure only.

  sumsq_np          sum of g^2 over the elements whose flag has bit1 set, and whether one of THOSE has all exponent bits set
  finalize_np       norm = grad_scale * sqrt(total); c = max_norm / (norm + 1e-6); coef = c if (max_norm > 0, finite, c < 1) else 1
                    (torch.nn.utils.clip_grad_norm_); skip = the non-finite flag.  `device_casts=True` adds the kernel's roundings:
                    grad_scale and max_norm arrive as fp32, norm and coef are stored as fp32.  `device_casts=False` keeps every
                    quantity in float64 (what test_grad_guard_host.py holds against torch on the CPU).
  guarded_adamw_np  oracle.optim.adamw_step on gradient * (grad_scale * coef), or nothing at all on a skipped step; returns the
                    number of applied updates, which is the `step` of the bias correction.
"""
import numpy as np
import torch

from oracle import optim as oopt

EXP_MASK = np.uint32(0x7F800000)


def sumsq_np(grad, flags):
    grad = np.asarray(grad).reshape(-1)
    if grad.dtype != np.float64:          # the device's gradients are fp32; float64 input is the all-double variant of the host test
        grad = grad.astype(np.float32)
    active = (np.asarray(flags).reshape(-1) & 2) != 0
    g = np.ascontiguousarray(grad[active])
    if g.dtype == np.float32:
        nonfinite = bool(((g.view(np.uint32) & EXP_MASK) == EXP_MASK).any())
    else:
        nonfinite = not bool(np.isfinite(g).all())
    with np.errstate(over="ignore", invalid="ignore"):
        g64 = g.astype(np.float64)
        return float(np.sum(g64 * g64)), nonfinite


def finalize_np(total, nonfinite, grad_scale, max_norm, device_casts=True):
    """-> (norm, coef, skip)"""
    gs, mx = float(grad_scale), float(max_norm)
    if device_casts:
        gs, mx = float(np.float32(gs)), float(np.float32(mx))
    with np.errstate(invalid="ignore"):
        norm = gs * float(np.sqrt(np.float64(total)))
        c = mx / (norm + 1e-6)
    clip = mx > 0 and np.isfinite(mx) and c < 1
    coef = c if clip else 1.0
    if device_casts:
        norm, coef = float(np.float32(norm)), float(np.float32(coef))
    return norm, coef, bool(nonfinite)


def guarded_adamw_np(params, grads, state, applied, lr, grad_scale, coef, skip, weight_decay, device_casts=True):
    """params / grads / state: dicts by name of torch CPU tensors (state[name] = (exp_avg, exp_avg_sq)); a gradient of None marks a
    parameter that takes no part (flag bit1 clear).  `applied` = updates applied so far.  Returns the new count."""
    if skip:
        return applied
    factor = float(np.float32(grad_scale) * np.float32(coef)) if device_casts else float(grad_scale) * float(coef)
    applied += 1
    for name, g in grads.items():
        if g is None:
            continue
        oopt.adamw_step(params[name], g * factor, state[name][0], state[name][1], applied, lr,
                        0.0 if oopt.is_no_decay(name) else weight_decay)
    return applied


def flat_of(grads, dtype=torch.float32):
    """The active gradients as one flat array with their flags: what the flat-buffer kernels see (inactive tensors contribute nothing)."""
    parts = [g.detach().reshape(-1).to(dtype).cpu().numpy() for g in grads.values() if g is not None]
    flat = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return flat, np.full(flat.shape, 2, np.uint8)
