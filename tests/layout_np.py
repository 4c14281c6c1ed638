"""Plain numpy / torch-CPU restatements of csrc/pk_layout.hip (weight packing, padded-twin boxes, row moves, DropPath, the input layout
conversion) and the helpers the layout tests share.  Nothing here touches a device or the package.

Everything in the unit is a copy, one fp32 add, one IEEE division or one round-to-nearest-even, so the comparisons are equalities of
bits, taken through integer views.  The bf16 reference is torch-CPU float32 -> bfloat16; tests/test_layout_host.py holds it to SPECIALS.
The one exception is the softplus-derivative path of the layout conversion (hardware exponential): `softplus_window` states its bar."""
import numpy as np
import torch

BF16_SENTINEL = 0x7FC1          # a bf16 NaN no conversion of a planted value produces
F32_SENTINEL = 0x7FC00123       # an fp32 NaN with a recognisable payload

# (fp32 bits, bf16 bits after round-to-nearest-even), written out by hand
SPECIALS = [
    (0x3F808000, 0x3F80),       # tie, even upper half: stays
    (0x3F818000, 0x3F82),       # tie, odd upper half: goes up to even
    (0xBF818000, 0xBF82),       # the same below zero
    (0x3F808001, 0x3F81),       # one above a tie
    (0x3F807FFF, 0x3F80),       # one below a tie
    (0x3F818001, 0x3F82),
    (0x3F817FFF, 0x3F81),
    (0x00000000, 0x0000),       # +0
    (0x80000000, 0x8000),       # -0
    (0x00000001, 0x0000),       # smallest fp32 subnormal
    (0x80000001, 0x8000),
    (0x00008000, 0x0000),       # subnormal tie, even upper half (zero)
    (0x00018000, 0x0002),       # subnormal tie, odd upper half
    (0x00400000, 0x0040),       # a subnormal that is a bf16 subnormal
    (0x007FFFFF, 0x0080),       # largest subnormal: rounds up to the smallest normal
    (0x7F7FFFFF, 0x7F80),       # largest finite: rounds to +inf
    (0xFF7FFFFF, 0xFF80),
    (0x7F800000, 0x7F80),       # +inf
    (0xFF800000, 0xFF80),       # -inf
]
SPECIAL_F32 = np.array([s for s, _ in SPECIALS], np.uint32)
SPECIAL_BF16 = np.array([b for _, b in SPECIALS], np.uint16)


def bf16_bits(a):
    """float32 array -> uint16 bits of its round-to-nearest-even bfloat16 (torch-CPU), same shape"""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(a.shape)


def bf16_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def special_positions(n, rng):
    """first, last and a few interior elements of a flat tensor of n elements, one position per special value where n allows"""
    k = len(SPECIALS)
    if n <= k:
        return np.arange(n)
    inner = 1 + rng.choice(n - 2, size=k - 2, replace=False)
    return np.concatenate([[0], inner, [n - 1]])


def plant_specials(a, rng, nan=True):
    """Overwrites elements of the float32 array `a` in place: SPECIALS at the first, the last and interior elements, and one quiet NaN
    (where `nan` and the tensor has room).  -> a"""
    flat = a.reshape(-1).view(np.uint32)
    pos = special_positions(flat.size, rng)
    order = np.concatenate([[0], rng.permutation(np.arange(1, len(SPECIALS) - 1)), [len(SPECIALS) - 1]])[:pos.size]
    flat[pos] = SPECIAL_F32[order]
    if nan and flat.size > 2 * len(SPECIALS):
        free = np.setdiff1d(np.arange(flat.size), pos)
        flat[free[free.size // 2]] = 0x7FC00000
    return a


def normal_with_specials(shape, rng, nan=True):
    return plant_specials(rng.standard_normal(shape).astype(np.float32), rng, nan)


def first_mismatch(got, ref, src_nan=None):
    """Flat index of the first element whose bits differ (a NaN of any payload passes where `src_nan` marks a NaN source), or None."""
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    bad = got != ref
    if src_nan is not None:
        src_nan = np.asarray(src_nan).reshape(-1)
        if got.dtype == np.uint16:
            is_nan = (got & 0x7FFF) > 0x7F80
        else:
            is_nan = (got & 0x7FFFFFFF) > 0x7F800000
        bad = np.where(src_nan, ~is_nan, bad)
    idx = np.flatnonzero(bad)
    return None if idx.size == 0 else int(idx[0])


def assert_bits(got, ref, what, src_nan=None):
    """Equality of bits through integer views; the message names the element and its 1024-element block."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.dtype.kind == "u", (got.dtype, ref.dtype)
    assert got.size == ref.size, f"{what}: {got.size} elements, reference {ref.size}"
    i = first_mismatch(got, ref, src_nan)
    if i is not None:
        n_bad = int((got.reshape(-1) != ref.reshape(-1)).sum())
        raise AssertionError(f"{what}: element {i} (block {i // 1024}) holds {int(got.reshape(-1)[i]):#x}, reference "
                             f"{int(ref.reshape(-1)[i]):#x}; {n_bad} of {got.size} elements differ")


# ------------------------------------------------------------------------------------------------ weight packing
def pack_shape(N, C, T, mode, Cp, Np):
    return (N, T, Cp) if mode == 0 else (C, T, Np) if mode == 1 else (C, Np)


def pack_ref(w, N, C, T, mode, Cp, Np):
    """fp32 source viewed as [N][C][T] -> float32 array in the packed layout, padded lanes +0 (the rounding is bf16_bits'):
    mode 0: dst[n][t][cp] = w[n][cp][t];  mode 1: dst[c][t][np] = w[np][c][T-1-t];  mode 2: dst[c][np] = w[np][c]"""
    w = np.asarray(w, np.float32).reshape(N, C, T)
    dst = np.zeros(pack_shape(N, C, T, mode, Cp, Np), np.float32)
    if mode == 0:
        dst[:, :, :C] = w.transpose(0, 2, 1)
    elif mode == 1:
        dst[:, :, :N] = w[:, :, ::-1].transpose(1, 2, 0)
    else:
        assert T == 1
        dst[:, :N] = w[:, :, 0].T
    return dst


def pack_ref_loops(w, N, C, T, mode, Cp, Np):
    """The table of the issue read literally, one element at a time (small sizes only): what pack_ref is held against."""
    w = np.asarray(w, np.float32).reshape(N, C, T)
    dst = np.zeros(pack_shape(N, C, T, mode, Cp, Np), np.float32)
    if mode == 0:
        for n in range(N):
            for t in range(T):
                for cp in range(Cp):
                    dst[n, t, cp] = w[n, cp, t] if cp < C else 0.0
    elif mode == 1:
        for c in range(C):
            for t in range(T):
                for np_ in range(Np):
                    dst[c, t, np_] = w[np_, c, T - 1 - t] if np_ < N else 0.0
    else:
        for c in range(C):
            for np_ in range(Np):
                dst[c, np_] = w[np_, c, 0] if np_ < N else 0.0
    return dst


def pack_pad_mask(N, C, T, mode, Cp, Np):
    """True at the padded lanes of a packed region"""
    m = np.zeros(pack_shape(N, C, T, mode, Cp, Np), bool)
    if mode == 0:
        m[..., C:] = True
    else:
        m[..., N:] = True
    return m


def up(n, k):
    return -(-n // k) * k


def block_table_ref(sizes, per_block):
    """-> (descriptor of each workgroup, first workgroup of that descriptor, number of workgroups), as lists"""
    blk_desc, blk_first = [], []
    for i, n in enumerate(sizes):
        first = len(blk_desc)
        k = (n + per_block - 1) // per_block
        for _ in range(k):
            blk_desc.append(i)
            blk_first.append(first)
    return blk_desc, blk_first, len(blk_desc)


# ------------------------------------------------------------------------------------------------ padded-twin boxes
def box_view(twin_flat, off, r, p):
    """The real tensor's box inside the flat twin: twin[off : off + prod(p)].reshape(p)[:r0, :r1, :r2, :r3] (a view)"""
    n = int(np.prod(p))
    return twin_flat[off:off + n].reshape(p)[:r[0], :r[1], :r[2], :r[3]]


def box_mask(total, rows):
    """True at every element of a flat twin of `total` elements that lies inside one of the boxes `rows` = [(off, r, p), ...]"""
    m = np.zeros(total, bool)
    for off, r, p in rows:
        box_view(m, off, r, p)[...] = True
    return m


def embed_by_name(name, real, twin_shape, heads=None):
    """The twin tensor that holds `real` (numpy), derived from the parameter's name and its block's head count alone: attention weights
    are head-structured (qkv rows (3, heads, d -> dp), proj columns (heads, d -> dp)), everything else is zero-extended at the end of
    every dimension.  -> (twin tensor with +0 padding, mask of the elements that belong to the real tensor)"""
    real = np.asarray(real)
    twin_shape = tuple(twin_shape)
    out, mask = np.zeros(twin_shape, real.dtype), np.zeros(twin_shape, bool)
    structured = heads is not None and real.shape != twin_shape
    if structured and name.endswith("attn.qkv.weight"):
        C, Cp = real.shape[1], twin_shape[1]
        d, dp = C // heads, Cp // heads
        assert real.shape == (3 * C, C) and twin_shape == (3 * Cp, Cp)
        o, m = out.reshape(3, heads, dp, Cp), mask.reshape(3, heads, dp, Cp)
        o[:, :, :d, :C] = real.reshape(3, heads, d, C)
        m[:, :, :d, :C] = True
    elif structured and name.endswith("attn.qkv.bias"):
        C, Cp = real.shape[0] // 3, twin_shape[0] // 3
        d, dp = C // heads, Cp // heads
        o, m = out.reshape(3, heads, dp), mask.reshape(3, heads, dp)
        o[:, :, :d] = real.reshape(3, heads, d)
        m[:, :, :d] = True
    elif structured and name.endswith("attn.proj.weight"):
        C, Cp = real.shape[0], twin_shape[0]
        d, dp = C // heads, Cp // heads
        o, m = out.reshape(Cp, heads, dp), mask.reshape(Cp, heads, dp)
        o[:C, :, :d] = real.reshape(C, heads, d)
        m[:C, :, :d] = True
    else:
        assert real.ndim == len(twin_shape) and all(a <= b for a, b in zip(real.shape, twin_shape)), (name, real.shape, twin_shape)
        sl = tuple(slice(0, s) for s in real.shape)
        out[sl] = real
        mask[sl] = True
    return out, mask


# ------------------------------------------------------------------------------------------------ row moves, DropPath
def rows_gather_ref(src, rowmap):
    """dst[r] = src[map[r]], all-zero bits where map[r] = -1; src, dst: (rows, dwords) uint32"""
    dst = src[np.maximum(rowmap, 0)]
    dst[rowmap < 0] = 0
    return dst


def rows_scatter_ref(src, rowmap, dst):
    """dst[map[r]] = src[r] for map[r] >= 0 (an injective map); every other row of `dst` stays.  -> a new array"""
    dst = dst.copy()
    keep = rowmap >= 0
    dst[rowmap[keep]] = src[keep]
    return dst


def drop_path_ref(x, mask, keep):
    """(x / keep) * mask[sample] in float32: one IEEE division, one multiplication"""
    x = np.asarray(x, np.float32)
    return (x / np.float32(keep)) * np.asarray(mask, np.float32).reshape(-1, *([1] * (x.ndim - 1)))


# ------------------------------------------------------------------------------------------------ input layout conversion
def nhwc_ref(x, Cpad):
    """(B,Cin,H,W) float32 -> (B,H,W,Cpad) float32, channels >= Cin +0 (the rounding is bf16_bits')"""
    B, Cin, H, W = x.shape
    y = np.zeros((B, H, W, Cpad), np.float32)
    y[..., :Cin] = x.transpose(0, 2, 3, 1)
    return y


def bf16_neighbours(r):
    """float64 r -> (lo, hi, dist): the bf16 values on either side of r (towards and away from zero, as float64, signed) and the distance
    from r to the nearest boundary of bf16 rounding (a midpoint between two adjacent bf16 values).  Normal range only."""
    a = np.abs(r)
    _, e = np.frexp(a)                              # a = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e-8)
    ulp = np.ldexp(1.0, e - 8)
    q = a / ulp                                     # in [128, 256)
    fl = np.floor(q)
    dist = np.abs(q - fl - 0.5)
    dist = np.minimum(dist, q - 127.75)             # the last midpoint of the binade below, whose ulp is half as wide
    sign = np.where(np.signbit(r), -1.0, 1.0)
    return sign * fl * ulp, sign * (fl + 1) * ulp, dist * ulp


def softplus_window(x, sp):
    """The bar of the softplus-derivative path, out = bf16(x (1 - exp(-sp))) with the hardware exponential.
    -> (rne, lo, hi, inside): uint16 bits of RNE_bf16(r) for the float64 r = x (1 - exp(-sp)), the bits of r's two bf16 neighbours, and
    the mask of the elements where r lies within 4 * 2^-23 * |x| of a rounding boundary.  Outside the mask the output must equal `rne`;
    inside it may be either neighbour.  The window allows about 4 units of 2^-24 absolute error in e = exp(-sp) <= 1, the fp32 subtraction
    and product roundings, and a factor of two on top.  It also contains every r whose float32 rounding could cross a boundary
    (|r| <= |x|), so `rne` may be taken through float32."""
    x64, sp64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(sp, np.float32).astype(np.float64)
    r = x64 * (1.0 - np.exp(-sp64))
    lo, hi, dist = bf16_neighbours(np.where(r == 0, 1.0, r))
    inside = (dist <= 4.0 * 2.0 ** -23 * np.abs(x64)) & (r != 0)
    rne = bf16_bits(r.astype(np.float32))
    return rne, bf16_bits(lo.astype(np.float32)), bf16_bits(hi.astype(np.float32)), inside
