"""numpy restatement of pk_activation_stats / pk_activation_quantiles (rules: include/posekernels.h, DESIGN.md "Activation statistics").

Inputs are bf16 BIT PATTERNS: (M, C) uint16.  Nothing here calls the library: the split of rows over workgroups, the key / bin rule and
the order of the fp64 sums are written out again from the documented rules, so that the kernels can be compared bit for bit."""
import numpy as np

RECORD = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("min", "<f4"), ("max", "<f4"), ("n", "<i8"), ("n_zero", "<i8"),
                   ("n_negative", "<i8"), ("n_nonfinite", "<i8"), ("reserved", "<i8")])
BINS = 4096
ZERO_BIN = 2048
THREADS, UNROLL, MAX_BLOCKS, FOLD = 256, 4, 512, 16


def to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def from_f32(values):
    """float32 -> bf16 bits, round to nearest even (finite values; inf / NaN keep their top bits)."""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nonfinite = (u & 0x7f800000) == 0x7f800000
    return np.where(nonfinite, (u >> 16).astype(np.uint16) | np.where((u & 0xffff) != 0, 0x40, 0).astype(np.uint16), r)


def is_nonfinite(bits):
    return (np.asarray(bits, np.uint16) & 0x7f80) == 0x7f80


def key_of(bits):
    """Sortable key: -0 first mapped to +0; sign set -> ~bits, else bits | 0x8000."""
    b = np.asarray(bits, np.uint16).astype(np.uint32)
    b = np.where(b == 0x8000, 0, b)
    return np.where(b & 0x8000, ~b & 0xffff, b | 0x8000).astype(np.uint32)


def value_of_key(key):
    k = np.asarray(key, np.uint32)
    return to_f32(np.where(k & 0x8000, k & 0x7fff, ~k & 0xffff).astype(np.uint16))


def bin_of(bits):
    return key_of(bits) >> 4


def bin_edges():
    """4097 float64 edges: bin b holds edges[b] <= x < edges[b + 1]; the bins of the inf / NaN patterns are bounded by -inf / +inf."""
    keys = np.arange(BINS + 1, dtype=np.uint32) << 4
    keys[-1] = 0xffff
    with np.errstate(invalid="ignore"):
        e = value_of_key(keys).astype(np.float64)
    e[np.isnan(e) & (np.arange(BINS + 1) < BINS // 2)] = -np.inf
    e[np.isnan(e)] = np.inf
    return e


def split(M, C):
    """(workgroups, rows per pass G, rows per slab): a function of (M, C) alone."""
    G = THREADS // (C // 8)
    slab = G * UNROLL
    return min(MAX_BLOCKS, max(1, -(-M // slab))), G, slab


def _ordered_sum(d, M, C):
    """Per-channel sum of the (M, C) float64 array in the kernels' order: thread (b, r) adds rows s slab + u G + r in ascending (s, u) to
    0.0, the workgroup adds r = 0 .. G - 1 from left to right, the finalize adds workgroups g, g + 16, ... in ascending order to 0.0 in each
    of 16 groups and then the groups 0 .. 15 from left to right.  (Rows past M are +0.0:
    adding +0.0 to an accumulator that starts at +0.0 never changes it.)"""
    B, G, slab = split(M, C)
    K = -(-(-(-M // slab)) // B)
    pad = np.zeros((K * B * slab, C), np.float64)
    pad[:M] = d
    per_thread = pad.reshape(K, B, UNROLL, G, C).transpose(1, 3, 0, 2, 4).reshape(B, G, K * UNROLL, C)
    t = np.cumsum(per_thread, axis=2)[:, :, -1, :]          # cumsum: strictly sequential
    w = np.cumsum(t, axis=1)[:, -1, :]
    fold = np.zeros((-(-B // FOLD) * FOLD, C), np.float64)
    fold[:B] = w
    groups = np.cumsum(fold.reshape(-1, FOLD, C), axis=0)[-1]          # group g: workgroups g, g + 16, ... in ascending order
    return np.cumsum(groups, axis=0)[-1]


def stats(bits, c_used=None):
    """-> (records (c_used,) RECORD, hist (4096,) int64) of one call without accumulation."""
    bits = np.asarray(bits, np.uint16)
    M, C = bits.shape
    c_used = C if c_used is None else c_used
    bad = is_nonfinite(bits)
    zero = (bits & 0x7fff) == 0
    f = to_f32(np.where(zero, 0, bits).astype(np.uint16))       # -0 read as +0
    d = to_f32(np.where(bad | zero, 0, bits).astype(np.uint16)).astype(np.float64)      # what does not take part adds +0.0
    rec = np.zeros(c_used, RECORD)
    rec["sum"] = _ordered_sum(d, M, C)[:c_used]
    rec["sumsq"] = _ordered_sum(d * d, M, C)[:c_used]
    with np.errstate(invalid="ignore"):
        rec["min"] = np.where(bad, np.float32(np.inf), f).min(axis=0)[:c_used]
        rec["max"] = np.where(bad, np.float32(-np.inf), f).max(axis=0)[:c_used]
    rec["n"] = M
    rec["n_zero"] = (zero & ~bad).sum(axis=0)[:c_used]
    rec["n_negative"] = (~bad & ~zero & ((bits & 0x8000) != 0)).sum(axis=0)[:c_used]
    rec["n_nonfinite"] = bad.sum(axis=0)[:c_used]
    used = bits[:, :c_used]
    hist = np.bincount(bin_of(used[~is_nonfinite(used)]).astype(np.int64), minlength=BINS).astype(np.int64)
    return rec, hist


def accumulate(old, new):
    """The accumulate rule: old + new per field, min / max combined.  old, new = (records, hist)."""
    (ro, ho), (rn, hn) = old, new
    r = np.zeros(len(ro), RECORD)
    for k in ("sum", "sumsq", "n", "n_zero", "n_negative", "n_nonfinite"):
        r[k] = ro[k] + rn[k]
    r["min"], r["max"] = np.minimum(ro["min"], rn["min"]), np.maximum(ro["max"], rn["max"])
    return r, ho + hn


def quantiles(bits, q, c_used=None):
    """-> (Q, 2) float32: v[lo], v[hi] of the sorted finite values of the channels < c_used (-0 as +0); NaN when there is none."""
    bits = np.asarray(bits, np.uint16)
    used = bits[:, :bits.shape[1] if c_used is None else c_used].reshape(-1)
    used = used[~is_nonfinite(used)]
    v = np.sort(to_f32(np.where((used & 0x7fff) == 0, 0, used).astype(np.uint16)))
    out = np.full((len(q), 2), np.nan, np.float32)
    n = v.size
    for i, qi in enumerate(q):
        if n == 0:
            continue
        pos = np.float64(qi) * np.float64(n - 1)
        lo = min(int(np.floor(pos)), n - 1)
        out[i] = v[lo], v[min(lo + 1, n - 1)]
    return out
