"""numpy restatement of the occlusion sensitivity units (csrc/pk_occlusion.hip; rules: DESIGN.md "Occlusion sensitivity"): the grid of
patch positions, the occluded copies of a packed image, the per-map summary in the kernel's exact summation order, and the map painted by
the LITERAL double loop of the reference (analysis/advanced_analysis.py:409-425, restated) next to the closed form the kernel uses."""
import numpy as np

F32, F64 = np.float32, np.float64
THREADS, WAVE = 256, 64
MEASURES = {"sum": 0, "max": 1, "shift": 2}

# (H, W, patch, stride): ragged and odd sizes, stride > patch, one row of positions, an empty grid, the flagship size
GRID_CASES = [(12, 10, 4, 3), (33, 25, 7, 3), (32, 24, 4, 8), (20, 15, 4, 8), (17, 40, 16, 8), (16, 16, 16, 8), (64, 48, 16, 16), (256, 192, 16, 8)]


# ------------------------------------------------------------------------------------------------ grid
def positions(extent, patch, stride):
    """The reference's loop bounds, literally."""
    return list(range(0, extent - patch, stride))


def count(extent, patch, stride):
    """The closed form of len(positions(...)): ceil((extent - patch) / stride) when extent > patch, else 0."""
    return -((patch - extent) // stride) if extent > patch else 0


def grid(H, W, patch, stride):
    return len(positions(H, patch, stride)), len(positions(W, patch, stride))


# ------------------------------------------------------------------------------------------------ occluded copies
def bf16_bits(v):
    """float32 -> the 16 bits of its bf16, round to nearest even (finite values and infinities)."""
    b = np.asarray(v, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def pack_image(chw):
    """(3,H,W) float32 -> (H,W,8) uint16: the stem's packed pixels, channels 3..7 zero."""
    out = np.zeros(chw.shape[1:] + (8,), np.uint16)
    out[..., :3] = np.moveaxis(bf16_bits(chw), 0, -1)
    return out


def occluded_copies(packed, patch, stride, fill=None):
    """(H,W,8) uint16 -> (P,H,W,8) uint16 in the order of the reference's loops: copy a * nx + b has the patch at (a stride, b stride)
    replaced by the fill (three floats rounded to bf16, or 0) with zero pad channels."""
    H, W, _ = packed.shape
    px = np.zeros(8, np.uint16)
    if fill is not None:
        px[:3] = bf16_bits(np.asarray(fill, F32))
    out = []
    for i in positions(H, patch, stride):
        for j in positions(W, patch, stride):
            c = packed.copy()
            c[i:i + patch, j:j + patch] = px
            out.append(c)
    return np.stack(out) if out else np.zeros((0, H, W, 8), np.uint16)


# ------------------------------------------------------------------------------------------------ summary
def fixed_order_sum(flat):
    """float64 sum in the kernel's order: thread t adds elements t, t + 256, ... in ascending order to 0.0; inside each wave of 64 threads
    the xor butterfly with offsets 32, 16, ..., 1; then wave 0 + wave 1 + wave 2 + wave 3 from left to right.  A NaN propagates."""
    v = np.asarray(flat, F32).astype(F64).reshape(-1)
    full, rest = len(v) // THREADS, len(v) % THREADS
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(THREADS)
        for chunk in v[:full * THREADS].reshape(full, THREADS):
            s = s + chunk
        if rest:                                                  # the ragged last round: only the first `rest` threads add anything
            s[:rest] = s[:rest] + v[full * THREADS:]
        s = s.reshape(THREADS // WAVE, WAVE)
        lanes = np.arange(WAVE)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        t = s[0, 0]
        for w in range(1, THREADS // WAVE):
            t = t + s[w, 0]
    return t


def summary(maps):
    """(..., h, w) float32 -> (..., 4) float64: sum (fixed order), max, argmax x, argmax y.  The first of equal maxima wins, a NaN never
    wins, a map with nothing above -inf reports -inf at index 0."""
    maps = np.asarray(maps, F32)
    h, w = maps.shape[-2:]
    flat = maps.reshape(-1, h * w)
    out = np.zeros((len(flat), 4))
    for m, row in enumerate(flat):
        cand = np.where(np.isnan(row), -np.inf, row)
        idx = int(np.argmax(cand))                                # the first index of the largest value; -0 == +0
        if not cand[idx] > -np.inf:
            idx, mx = 0, -np.inf
        else:
            mx = F64(row[idx])
        out[m] = fixed_order_sum(row), mx, idx % w, idx // w
    return out.reshape(maps.shape[:-2] + (4,))


# ------------------------------------------------------------------------------------------------ the map
def values(base, table, measure):
    """(K,4), (P,K,4) -> (P,K) float64: what the reference calls `sensitivity` for every copy and joint."""
    base, table = np.asarray(base, F64), np.asarray(table, F64)
    m = MEASURES[measure] if isinstance(measure, str) else measure
    if m == 0:
        return base[None, :, 0] - table[:, :, 0]
    if m == 1:
        return base[None, :, 1] - table[:, :, 1]
    dx, dy = table[:, :, 2] - base[None, :, 2], table[:, :, 3] - base[None, :, 3]
    return np.sqrt(dx * dx + dy * dy)


def paint_loop(vals, H, W, patch, stride):
    """The reference's loop, literally: (P,K) -> (K,H,W); later positions overwrite earlier ones."""
    K = vals.shape[1]
    out = np.zeros((K, H, W))
    p = 0
    for i in range(0, H - patch, stride):
        for j in range(0, W - patch, stride):
            out[:, i:i + patch, j:j + patch] = vals[p][:, None, None]
            p += 1
    assert p == len(vals)
    return out


def paint_closed(vals, H, W, patch, stride):
    """The gather form: pixel (y, x) has a = min(y // stride, ny - 1), b = min(x // stride, nx - 1), is covered iff y < a stride + patch and
    x < b stride + patch, and then takes copy a nx + b; otherwise 0."""
    K = vals.shape[1]
    ny, nx = grid(H, W, patch, stride)
    out = np.zeros((K, H, W))
    if ny == 0 or nx == 0:
        return out
    a = np.minimum(np.arange(H) // stride, ny - 1)
    b = np.minimum(np.arange(W) // stride, nx - 1)
    cover = (np.arange(H) < a * stride + patch)[:, None] & (np.arange(W) < b * stride + patch)[None, :]
    src = a[:, None] * nx + b[None, :]
    out[:] = np.where(cover[None], np.moveaxis(vals[src], -1, 0), 0.0)
    return out
