"""numpy restatement of the weight EMA that pk_adamw_step_ema (csrc/pk_optim.hip) keeps next to the AdamW update, for the tests and
scripts/bench_ema_step.py.  Test infrastructure only.

  decay_np        d_t = min(decay, (1 + t) / (10 + t)); t = applied updates so far, this one included (the bias correction's t, >= 1).
  ema_update_np   e + (1 - d_t) * (p_new - e) on the elements whose flag has bit1 set; every other element is returned as it came.
  ema_closed_np   the same average written without the recurrence: e_T = prod_t d_t * e_0 + sum_t (1 - d_t) * prod_{s>t} d_s * p_t.

`device_casts=False` keeps every quantity in float64.  `device_casts=True` is the kernel's arithmetic: t, decay, the quotient, d_t, 1 - d_t
and the three operations of the update are each rounded to fp32 (the library is built without FMA contraction), so it returns float32.
"""
import numpy as np


def decay_np(t, decay, device_casts=False):
    if device_casts:
        f = np.float32
        return f(min(f(decay), f(f(1.0) + f(t)) / f(f(10.0) + f(t))))
    return min(float(decay), (1.0 + float(t)) / (10.0 + float(t)))


def ema_update_np(e, p_new, t, decay, flags=None, device_casts=False):
    d = decay_np(t, decay, device_casts)
    if device_casts:
        e, p_new = np.asarray(e, np.float32), np.asarray(p_new, np.float32)
        w = np.float32(np.float32(1.0) - d)
        with np.errstate(all="ignore"):
            out = (e + w * (p_new - e)).astype(np.float32)
    else:
        e, p_new = np.asarray(e, np.float64), np.asarray(p_new, np.float64)
        with np.errstate(all="ignore"):
            out = e + (1.0 - d) * (p_new - e)
    if flags is not None:
        out = np.where((np.asarray(flags) & 2) != 0, out, e)
    return out


def ema_closed_np(e0, ps, decay):
    """ps[k] = the weights after update t = k + 1.  float64 throughout."""
    ds = [decay_np(t, decay) for t in range(1, len(ps) + 1)]
    out = float(np.prod(ds)) * np.asarray(e0, np.float64)
    for k, p in enumerate(ps):
        out = out + (1.0 - ds[k]) * float(np.prod(ds[k + 1:])) * np.asarray(p, np.float64)
    return out
