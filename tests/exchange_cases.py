"""Case tables, inputs and error bounds of the exchange-unit kernel tests (tests/test_gpu_exchange_kernels.py runs them on the device,
tests/test_exchange_host.py holds the tables against the launch arithmetic and shows that the bounds can fail).

Every case is the smallest shape that reaches its path; the tables DECLARE the plan (workgroups and trips of the grid-stride loop, the
lanes per chunk of the backward) and the host test holds the declaration against exchange_np.fuse_plan / upsample_plan.

Bound, per element:  |got - ref| <= 2^-8 |ref| + a,  a = (1 + 2^-8) E,  E = k U mag,  U = 2^-24.
  The kernels accumulate in fp32 and round once to bf16.  With c = ref + e, |e| <= E, the fp32 value, the store adds at most half a bf16
  ulp of c, which is at most 2^-8 |c| <= 2^-8 (|ref| + E); hence a.  `mag` is the sum of the magnitudes of the products the element adds
  (the same weights applied to |input|: exchange_np's magnitude=True), so E scales with the input magnitudes of the case, and k counts the
  fp32 roundings one product can pass through, plus one for the second-order terms:
    fused sum        k = 5 + n    an up-sampled tap passes (v (1 - fx) + v' fx) (1 - fy) + (..) fy: two multiplications and two additions,
                                  then at most n additions into the accumulator of n terms (the float32 (1 - f) is part of the
                                  specification, the reference uses it too; the ReLU is 1-Lipschitz and adds nothing)
    backward         k = n + 7    wy wx and (wy wx) v: two multiplications; a lane adds at most n terms, the butterfly over the up to 16
                                  lanes of a chunk adds four more levels; n = the number of output pixels with a weight on the source
                                  pixel (at most 16 x 16 at ratio 8)
  Nothing here is taken from what the kernels return."""
import numpy as np

import exchange_np as xn

U = xn.U


class Fuse:
    """One fused sum: sizes = [(Hi, Wi)] of its inputs.  single / grouped: (workgroups, trips) under the cap of a single launch (4096)
    and of a group member (2048)."""

    def __init__(self, name, B, H, W, C, sizes, relu, single, grouped, mask=False, seed=0):
        self.name, self.B, self.H, self.W, self.C, self.sizes, self.relu = name, B, H, W, C, list(sizes), relu
        self.single, self.grouped, self.mask, self.seed = single, grouped, mask, seed

    def data(self):
        """-> (inputs, mask_y or None): float32 arrays of bf16 values; N(0, 1), every third case scaled by 16"""
        rng = np.random.default_rng(1000 + self.seed)
        scale = 16.0 if self.seed % 3 == 2 else 1.0
        ins = [xn.bf16_values(rng.standard_normal((self.B, h, w, self.C)) * scale) for h, w in self.sizes]
        return ins, (mask_values((self.B, self.H, self.W, self.C), rng) if self.mask else None)

    def reference(self, ins, mask):
        ref = xn.fuse_sum_ref(ins, self.H, self.W, self.relu, mask)
        mag = xn.fuse_sum_ref(ins, self.H, self.W, self.relu, mask, magnitude=True)
        return ref, bound(ref, (5 + len(ins)) * U * mag)


class Up:
    """One up-sampling backward (H, W) -> (Hs, Ws).  split: lanes per chunk; single / grouped: (workgroups, trips) as above; positive: dy
    drawn from [1, 2), so that no missing tap can cancel."""

    def __init__(self, name, B, H, W, Hs, Ws, C, split, single, grouped, positive=False, seed=0):
        self.name, self.B, self.H, self.W, self.Hs, self.Ws, self.C = name, B, H, W, Hs, Ws, C
        self.split, self.single, self.grouped, self.positive, self.seed = split, single, grouped, positive, seed

    def data(self):
        """-> (dy, mask_y): float32 arrays of bf16 values"""
        rng = np.random.default_rng(2000 + self.seed)
        shape = (self.B, self.H, self.W, self.C)
        dy = rng.uniform(1.0, 2.0, shape) if self.positive else rng.standard_normal(shape) * (16.0 if self.seed % 3 == 2 else 1.0)
        return xn.bf16_values(dy), mask_values(shape, rng)

    def reference(self, dy, mask):
        ref = xn.upsample_bwd_ref(dy, self.Hs, self.Ws, mask)
        mag = xn.upsample_bwd_ref(dy, self.Hs, self.Ws, mask, magnitude=True)
        n = xn.upsample_bwd_terms(self.H, self.W, self.Hs, self.Ws)[None, :, :, None]
        return ref, bound(ref, (n + 7) * U * mag)


def bound(ref, E):
    return 2.0 ** -8 * np.abs(ref) + (1 + 2.0 ** -8) * E


def mask_values(shape, rng):
    """A ReLU output as the kernels read it: half of it positive, the rest zeros, -0.0 and negatives (none of which may pass)."""
    pool = np.array([0.75, 2.0, 3.0e-3, 0.0, -0.0, -1.5], np.float32)
    return xn.bf16_values(pool[rng.integers(0, len(pool), shape)])


# ================================================================================================ fused sum
FUSE = [
    Fuse("one term, C = 8", 2, 5, 3, 8, [(5, 3)], 1, (1, 1), (1, 1)),
    Fuse("two same-size terms, 567 chunks", 3, 9, 7, 24, [(9, 7), (9, 7)], 0, (3, 1), (3, 1)),
    Fuse("ratios 2 / 4 / 8, C = 24", 2, 16, 24, 24, [(16, 24), (8, 12), (4, 6), (2, 3)], 1, (9, 1), (9, 1)),
    Fuse("9x7 <- 5x4", 1, 9, 7, 8, [(9, 7), (5, 4)], 0, (1, 1), (1, 1)),
    Fuse("13x13 <- 12x12, C = 24", 2, 13, 13, 24, [(13, 13), (12, 12)], 1, (4, 1), (4, 1)),
    Fuse("65x49 <- 33x25 <- 17x13 <- 9x7", 2, 65, 49, 8, [(65, 49), (33, 25), (17, 13), (9, 7)], 1, (25, 1), (25, 1)),
    Fuse("three terms, the first one up-sampled", 1, 9, 7, 24, [(5, 4), (9, 7), (3, 2)], 0, (1, 1), (1, 1)),
    Fuse("one up-sampled term alone", 2, 13, 13, 8, [(12, 12)], 0, (2, 1), (2, 1)),
    Fuse("one chunk", 1, 1, 1, 8, [(1, 1)], 0, (1, 1), (1, 1)),
]
for _i, _c in enumerate(FUSE):
    _c.seed = _i
# 1 052 415 chunks, 3 839 past 4096 x 256: the single launch takes a second, partly empty trip; cchunks = 257
FUSE_WRAP = Fuse("single launch wraps", 1, 65, 63, 2056, [(65, 63), (33, 32)], 1, (4096, 2), None, seed=20)
# 528 255 chunks, 3 967 past 2048 x 256: wraps as a group member only; cchunks = 129
FUSE_WRAP_GROUPED = Fuse("group member wraps", 1, 65, 63, 1032, [(65, 63), (33, 32)], 1, (2064, 1), (2048, 2), seed=21)
# the wrapped member between one-chunk and tiny members: the member search of the grouped kernel at every kind of boundary
FUSE_WRAP_GROUP = [FUSE[0], FUSE[8], FUSE_WRAP_GROUPED, FUSE[8], FUSE[3]]
# mask_y (group form only): term 0 masked; as the backward uses it (same-size terms) and with up-sampled terms behind the masked one
FUSE_MASKED = [
    Fuse("masked, three same-size terms", 2, 9, 7, 24, [(9, 7), (9, 7), (9, 7)], 0, None, (2, 1), mask=True, seed=30),
    Fuse("masked, one term", 1, 5, 3, 8, [(5, 3)], 0, None, (1, 1), mask=True, seed=31),
    Fuse("masked, up-sampled terms behind it, ReLU", 2, 13, 13, 8, [(13, 13), (12, 12), (7, 4)], 1, None, (2, 1), mask=True, seed=32),
]

# ================================================================================================ up-sampling backward
UP = [
    # exact even ratios: the 2r-row window
    Up("ratio 2", 2, 16, 12, 8, 6, 24, 1, (2, 1), (2, 1), positive=True),
    Up("ratio 4", 2, 16, 24, 4, 6, 8, 4, (1, 1), (1, 1)),
    Up("ratio 8", 2, 32, 24, 4, 3, 24, 16, (5, 1), (5, 1), positive=True),
    Up("ratio 6: 1/6 is not a float32", 3, 12, 12, 2, 2, 8, 4, (1, 1), (1, 1)),
    # ratios that are not integers: the generic window, at sizes whose contributors it contains (exchange_np.gather_window: KNOWN GAP --
    # 13 <- 12, 19 <- 6, 65 <- 9 are not among them and are not tested here)
    Up("33x17 <- 17x9", 1, 33, 17, 17, 9, 8, 1, (1, 1), (1, 1), positive=True),
    Up("11 <- 3", 1, 11, 11, 3, 3, 8, 4, (1, 1), (1, 1)),
    Up("19 <- 5", 2, 19, 19, 5, 5, 8, 4, (1, 1), (1, 1), positive=True),
    Up("65x49 <- 17x13", 2, 65, 49, 17, 13, 8, 4, (7, 1), (7, 1), positive=True),
    Up("67x53 <- 9x7", 2, 67, 53, 9, 7, 8, 16, (8, 1), (8, 1), positive=True),
    Up("7x67 <- 4x9", 1, 7, 67, 4, 9, 8, 1, (1, 1), (1, 1), positive=True),
    Up("67x7 <- 9x4", 1, 67, 7, 9, 4, 8, 16, (3, 1), (3, 1)),
    Up("11x65 <- 3x17", 1, 11, 65, 3, 17, 8, 4, (1, 1), (1, 1), positive=True),
    Up("65x11 <- 17x3", 1, 65, 11, 17, 3, 8, 4, (1, 1), (1, 1)),
    # ratio 1 and an odd integer ratio take the generic window too
    Up("ratio 1", 2, 7, 5, 7, 5, 24, 1, (1, 1), (1, 1)),
    Up("ratio 3", 2, 9, 15, 3, 5, 8, 1, (1, 1), (1, 1), positive=True),
    Up("ratio 1 x 2", 1, 7, 10, 7, 5, 8, 1, (1, 1), (1, 1)),
]
for _i, _c in enumerate(UP):
    _c.seed = _i
# the last trip of a group member (2048 workgroups) partly off: 131 124 chunks = 131 072 + 52 at 4 lanes per chunk, 32 805 = 32 768 + 37
# at 16 (37 chunks end inside a wavefront).  The ratio is in H alone (the plan looks at nothing else), so dy stays at a few million elements
UP_PARTIAL = [
    Up("split 4, second trip of 52 chunks", 28, 12, 7, 3, 7, 1784, 4, (2049, 1), (2048, 2), positive=True, seed=40),
    Up("split 16, second trip of 37 chunks", 3, 72, 5, 9, 5, 1944, 16, (2051, 1), (2048, 2), positive=True, seed=41),
]
LAST_TRIP = {"split 4, second trip of 52 chunks": 52, "split 16, second trip of 37 chunks": 37}


# ================================================================================================ dropped contributors
def up_contributions(c, dy, mask, b, ys, xs, ch):
    """float64 (H, W): what every output pixel adds to dsrc[b, ys, xs, ch] -- the scatter written out for ONE element, from the taps."""
    g = np.where(mask[b, :, :, ch] > 0, dy[b, :, :, ch], 0).astype(np.float64) if mask is not None else dy[b, :, :, ch].astype(np.float64)
    out = np.zeros((c.H, c.W))
    for oy in range(c.H):
        y0, y1, fy = xn.bil_taps(oy, c.Hs, c.H)
        wy = np.float32((np.float32(1) - fy if y0 == ys else 0) + (fy if y1 == ys else 0))
        if wy == 0:
            continue
        for ox in range(c.W):
            x0, x1, fx = xn.bil_taps(ox, c.Ws, c.W)
            wx = np.float32((np.float32(1) - fx if x0 == xs else 0) + (fx if x1 == xs else 0))
            out[oy, ox] = float(wy) * float(wx) * g[oy, ox]
    return out


def fuse_contributions(c, ins, mask, b, y, x, ch):
    """list of float64: every product that out[b, y, x, ch] adds (before the ReLU), from the taps."""
    out = []
    for k, t in enumerate(ins):
        if t.shape[1] == c.H and t.shape[2] == c.W:
            v = float(t[b, y, x, ch])
            out.append(v if not (k == 0 and mask is not None and not mask[b, y, x, ch] > 0) else 0.0)
            continue
        y0, y1, fy = xn.bil_taps(y, t.shape[1], c.H)
        x0, x1, fx = xn.bil_taps(x, t.shape[2], c.W)
        for yy, wy in ((y0, np.float32(1) - fy), (y1, fy)):
            for xx, wx in ((x0, np.float32(1) - fx), (x1, fx)):
                out.append(float(wy) * float(wx) * float(t[b, yy, xx, ch]))
    return out


def sample_elements(shape, seed, n=24):
    """n seeded element indices of an NHWC tensor, the first and the last element among them."""
    rng = np.random.default_rng(seed)
    picks = [tuple(0 for _ in shape), tuple(s - 1 for s in shape)]
    while len(picks) < n:
        picks.append(tuple(int(rng.integers(0, s)) for s in shape))
    return picks
