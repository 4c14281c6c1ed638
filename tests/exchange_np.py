"""numpy restatement of the exchange unit (csrc/pk_exchange.hip): the bilinear taps in float32 operation for operation as the kernels
form them, the gather window of upsample_bwd_body and the launch plans of chunk_grid / upsample_plan as integers, and float64
references of the fused sum and of the up-sampling backward.

The references take their WEIGHTS from the float32 taps (the kernels' own specification: the scale n_in / n_out is one float32 division)
and do everything else in float64.  The backward is the transpose of the forward over ALL output pixels -- no gather window -- written
with one weight matrix per axis: dsrc[b, ys, xs, c] = sum_oy sum_ox Wy[oy, ys] Wx[ox, xs] dy[b, oy, ox, c].  upsample_bwd_windowed is the
same sum restricted to a window function, i.e. what a kernel that scans only that window computes.

Tensors are numpy arrays in NHWC, (B, H, W, C); bf16_values() makes float32 data exactly representable in bf16."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24            # unit round-off of the fp32 accumulation
CHUNK_GRID_CAP, CHUNK_GRID_CAP_GROUPED = 4096, 2048
GROUP_MAX = 12


# ------------------------------------------------------------------------------------------------ taps and windows
def bil_taps(o, n_in, n_out):
    """Output index (or array of them) o of n_out -> (i0, i1, f): source taps and the float32 weight f of i1 (1 - f of i0), align_corners
    = False.  float32, one rounding per operation: s = (o + 0.5) * (n_in / n_out) - 0.5, clamped at 0 (no contraction into an fma)."""
    o = np.asarray(o)
    scale = F32(n_in) / F32(n_out)
    s = (o.astype(F32) + F32(0.5)) * scale - F32(0.5)
    s = np.maximum(s, F32(0))
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    f = s - i0.astype(F32)
    assert s.dtype == F32 and f.dtype == F32
    return i0, i1, f


def backward_weights(n_in, n_out):
    """float32 (n_out, n_in): W[o, i] = (i0 == i ? 1 - f : 0) + (i1 == i ? f : 0), the weight upsample_bwd_body gives output o on source i
    (both taps land on the last source where the border clamps them together: one float32 addition, as in the kernel)."""
    o = np.arange(n_out)
    i0, i1, f = bil_taps(o, n_in, n_out)
    W = np.zeros((n_out, n_in), F32)
    W[o, i0] = F32(1) - f
    W[o, i1] = W[o, i1] + f          # i1 == i0: (1 - f) + f in float32; i1 != i0: 0 + f
    return W


def forward_weights(n_in, n_out):
    """float64 (n_out, n_in) from the float32 taps: fuse_sum_body multiplies the value at i0 by the float32 (1 - f) and the one at i1 by f
    and adds the PRODUCTS, so clamped-together taps are summed here in float64."""
    o = np.arange(n_out)
    i0, i1, f = bil_taps(o, n_in, n_out)
    W = np.zeros((n_out, n_in), F64)
    np.add.at(W, (o, i0), (F32(1) - f).astype(F64))
    np.add.at(W, (o, i1), f.astype(F64))
    return W


def gather_window(ys, H, Hs):
    """(lo, hi): the output rows upsample_bwd_body scans for source row ys (an integer or an array of them), as integers exactly as the
    kernel forms them; the same expression serves columns.  Exact even ratio r: the 2r rows [ys r - r/2, ys r + 3r/2); otherwise from
    (ys - 1) r - 1 to (ys + 2) r + 1 with r = ceil(H / Hs); both clipped to [0, H].
    KNOWN GAP: the generic window contains every contributor where the ratio is an integer (support() shows it for every H <= 200).
    Where it is not, r over-estimates H / Hs and the lower bound overtakes the first contributor as ys grows: 13 <- 12 scans source row
    11 from output row 19 of 13 (nothing), 65 <- 9 scans source row 8 from row 55 while row 54 carries weight 0.046.  16 447 of the
    20 100 pairs 1 <= Hs <= H <= 200 lose a contributor that way; a lower bound formed with floor(H / Hs) loses none.  The configured
    pyramids have exact even ratios.  The device tests keep to shapes whose contributors this window contains."""
    r = (H + Hs - 1) // Hs
    if H == Hs * r and not (r & 1):
        return np.maximum(0, ys * r - r // 2), np.minimum(H, ys * r + 3 * r // 2)
    return np.maximum(0, (ys - 1) * r - 1), np.minimum(H, (ys + 2) * r + 1)


def window_covers(H, Hs):
    """True where gather_window contains every output row with a non-zero float32 weight, for every source row of Hs <- H."""
    first, last = support(H, Hs)
    lo, hi = gather_window(np.arange(Hs), H, Hs)
    return bool(((first >= lo) & (last < hi)).all())


def support(H, Hs):
    """-> (first, last), int arrays (Hs,): the first and the last output row whose float32 weight on each source row is non-zero
    (first > last where a source row has no contributor at all; with H >= Hs there is none)."""
    o = np.arange(H)
    i0, i1, f = bil_taps(o, Hs, H)
    first, last = np.full(Hs, H), np.full(Hs, -1)
    w0 = np.where(i0 == i1, (F32(1) - f) + f, F32(1) - f)
    for i, w in ((i0, w0), (i1, f)):
        on = w != 0
        np.minimum.at(first, i[on], o[on])
        np.maximum.at(last, i[on], o[on])
    return first, last


# ------------------------------------------------------------------------------------------------ launch plans
def chunk_grid(chunks, lanes, cap):
    """Workgroups of a grid-stride launch over `chunks` 16-byte chunks, `lanes` of 256 lanes per chunk, at most `cap`."""
    return min(cap, (chunks * lanes + 255) // 256)


def fuse_plan(B, H, W, C, cap):
    """-> (chunks, workgroups, trips of the grid-stride loop) of one fused sum."""
    chunks = B * H * W * (C // 8)
    blocks = chunk_grid(chunks, 1, cap)
    return chunks, blocks, -(-chunks // (blocks * 256))


def upsample_plan(B, H, Hs, Ws, C, cap):
    """-> (chunks, split, workgroups, trips, chunks of the last trip) of one up-sampling backward, as upsample_plan and upsample_bwd_body
    form them: `split` lanes share a chunk when the window is tall (ceil(H / Hs) >= 4 / 8) and the chunks are few."""
    chunks = B * Hs * Ws * (C // 8)
    ry = (H + Hs - 1) // Hs
    split = 16 if (ry >= 8 and chunks < (1 << 20)) else (4 if (ry >= 4 and chunks < (1 << 20)) else 1)
    blocks = chunk_grid(chunks, split, cap)
    per_trip = blocks * 256 // split
    trips = -(-chunks // per_trip)
    return chunks, split, blocks, trips, chunks - (trips - 1) * per_trip


# ------------------------------------------------------------------------------------------------ data
def bf16_values(x):
    """float32 array -> the same values with the low 16 bits cleared: exactly representable in bf16."""
    x = np.ascontiguousarray(x, F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def _along(A, x, axis):
    """Contract the LAST axis of matrix A (n_new, n_old) with `axis` of x; the new axis takes its place."""
    return np.moveaxis(np.tensordot(A, x, axes=([1], [axis])), 0, axis)


def _masked(x, mask):
    return x if mask is None else np.where(np.asarray(mask) > 0, x, 0)          # -0.0, negatives and NaN do not pass


# ------------------------------------------------------------------------------------------------ references
def fuse_sum_ref(inputs, H, W, relu, mask_y=None, magnitude=False):
    """float64 (B, H, W, C): relu?(sum_i up_i(inputs[i])), inputs (B, Hi, Wi, C) with Hi <= H, Wi <= W; an input of the output's size is
    added as it is, any other bilinearly up-sampled; mask_y (shape of the output): input 0 counts only where mask_y > 0.
    magnitude=True: sum_i up_i(|inputs[i]|) instead, without the ReLU: the sum of the magnitudes of every product the kernel adds."""
    out = None
    for k, x in enumerate(inputs):
        x = np.asarray(x, F64)
        if magnitude:
            x = np.abs(x)
        if x.shape[1] == H and x.shape[2] == W:
            t = _masked(x, mask_y) if k == 0 else x
        else:
            assert not (k == 0 and mask_y is not None), "the masked term must have the output's size"
            t = _along(forward_weights(x.shape[2], W), _along(forward_weights(x.shape[1], H), x, 1), 2)
        out = t if out is None else out + t
    return np.maximum(out, 0) if (relu and not magnitude) else out


def upsample_bwd_ref(dy, Hs, Ws, mask_y=None, magnitude=False, window=None):
    """float64 (B, Hs, Ws, C): the transpose of the bilinear up-sampling (Hs, Ws) -> dy's (H, W), summed over ALL output pixels.  mask_y
    (shape of dy): dy counts only where mask_y > 0.  magnitude=True: the same sum over |dy|.  window (see upsample_bwd_windowed)."""
    dy = np.asarray(dy, F64)
    _, H, W, _ = dy.shape
    g = _masked(np.abs(dy) if magnitude else dy, mask_y)
    Wy, Wx = backward_weights(Hs, H).astype(F64), backward_weights(Ws, W).astype(F64)
    if window is not None:
        for A, n_out, n_in in ((Wy, H, Hs), (Wx, W, Ws)):
            for s in range(n_in):
                lo, hi = window(s, n_out, n_in)
                A[:max(lo, 0), s] = 0
                A[max(hi, 0):, s] = 0
    return _along(Wx.T, _along(Wy.T, g, 1), 2)


def upsample_bwd_windowed(dy, Hs, Ws, window, mask_y=None):
    """What a gather kernel computes that scans, per axis, only the outputs lo <= o < hi with (lo, hi) = window(source index, n_out, n_in)."""
    return upsample_bwd_ref(dy, Hs, Ws, mask_y, window=window)


def upsample_bwd_terms(H, W, Hs, Ws):
    """(Hs, Ws) int: how many output pixels have a non-zero weight on each source pixel."""
    ny = (backward_weights(Hs, H) != 0).sum(0)
    nx = (backward_weights(Ws, W) != 0).sum(0)
    return ny[:, None] * nx[None, :]
