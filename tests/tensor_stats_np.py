"""numpy restatement of the per-tensor statistics record of pk_tensor_stats (csrc/pk_tensor_stats.hip), for the tests: per tensor the
record's fields from float64 arithmetic, with the three sums taken by math.fsum (correctly rounded, so "the exact value" up to one
rounding).  The derived values (mean, std, ...) are NOT restated here: the tests import hipops.derive_tensor_stats from the package."""
import math

import numpy as np

FIELDS = ("sum", "sumsq", "sumabs", "min", "max", "n", "nonfinite", "small", "zero")


def record_np(x, flags=None, tiny=0.0):
    """The record of one tensor: x float32 (any shape), flags uint8 per element or None (bit1 = takes part), tiny >= 0."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    take = np.ones(x.size, bool) if flags is None else (np.asarray(flags, np.uint8).reshape(-1) & 2) != 0
    part = x[take]
    bad = (part.view(np.uint32) & 0x7f800000) == 0x7f800000          # exponent bits all ones: inf / NaN
    fin = part[~bad].astype(np.float64)
    return {"sum": math.fsum(fin), "sumsq": math.fsum(fin * fin),          # the square of a float32 is exact in float64
            "sumabs": math.fsum(np.abs(fin)),
            "min": np.float32(fin.min()) if fin.size else np.float32(np.inf),
            "max": np.float32(fin.max()) if fin.size else np.float32(-np.inf),
            "n": int(part.size), "nonfinite": int(bad.sum()), "small": int((np.abs(fin) <= np.float64(np.float32(tiny))).sum()), "zero": 0}


def pack(tensors, poison=True):
    """Tensors -> (flat float32 buffer, offsets, counts): every tensor at a multiple of 4 elements; the padding behind a tensor is
    poisoned alternately with NaN and 1e38, so that one padding element read into a record shows in it."""
    offsets, off = [], 0
    for t in tensors:
        offsets.append(off)
        off += -(-t.size // 4) * 4
    flat = np.zeros(off, np.float32)
    pad = np.ones(off, bool)
    for t, o in zip(tensors, offsets):
        flat[o:o + t.size] = np.asarray(t, np.float32).reshape(-1)
        pad[o:o + t.size] = False
    idx = np.flatnonzero(pad)
    if poison:
        flat[idx] = np.where(np.arange(idx.size) % 2 == 0, np.float32(np.nan), np.float32(1e38))
    return flat, offsets, [int(t.size) for t in tensors]


def sum_bound(n, abs_sum):
    """Any order of n float64 additions of terms with absolute sum `abs_sum` is within (n - 1) u abs_sum / (1 - (n - 1) u) of the true sum,
    u = 2^-53 (Higham, Accuracy and Stability, eq. 4.4); n 2^-52 abs_sum covers it for every n < 2^50 and also the one rounding of fsum."""
    return n * 2.0 ** -52 * abs_sum
