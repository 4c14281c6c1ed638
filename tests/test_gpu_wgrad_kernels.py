"""Every weight-gradient kernel of csrc/pk_wgrad.hip where its slices and tiles end, against float64.

Which kernel, tile and slice count a weight gradient gets follows from its shape alone (wgrad_route / wgrad_group_route), so every case
of the tables below is a shape chosen for the edge it reaches: a ragged last M-slice, a second group of eight slices with its padding
workgroups, a last n- or c-tile a few columns wide, a tap boundary inside a column tile, slices that start in the middle of an image row.
The tables state kernel, tile, mode and slice count S of every case; test_case_tables_match_the_library (no device needed) holds S
against pk_wgrad_slices / pk_wgrad_group_slices and the set of cases against the instantiations that pk_wgrad.hip launches.  Entries are
called through the C-ABI directly.

Two passes per case, both against a float64 reference built from strided slices of the zero-padded input (no shared index arithmetic):
  * exact: x and g hold small integers (even channels from {0..3}, odd ones from {-3..3}), per-sample scales come from {0, 0.5, 1, 2}.
    Every product and every partial sum is a multiple of 0.5 far below 2^24, so the fp32 accumulation, the slab sums and the bias sums
    are exact in any order: dw, dbias and the float64 sum of the slabs must EQUAL the reference.  One dropped, doubled or misplaced row,
    tap or pad pixel changes an integer; sums in the non-negative channels pass 2^11, so a 16-bit round trip of a partial sum fails too;
  * real: bf16 data with a scale per channel spread over 10^-2 .. 10^2, row scales including 0 and 1/0.9; the reference re-rounds the
    scaled G rows to bf16 once, as the kernels do.  Per element, with U = 2^-24:  |error| <= (M + S + 16) U sum_m |g[m][n]| |x[m][c]|
    (M non-zero fp32 additions in any order, S for the slab sum, 16 for the lane combine of the reduction; the same with |g| for dbias).

Guards in both passes: x and g are views into larger buffers whose rows before and after (one sample's worth) are NaN, as are the rows
an arbitrary row map never names; the workspace is NaN up to its documented size and followed by 1024 sentinel floats; dw and dbias
start as NaN and are followed by sentinels.  A lane that reads a row it should not, or a write that is dropped or lands outside, fails.
"""
import os
import re

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
NAN = float("nan")
SENT = 12345.5          # sentinel value (exact in fp32)
WS = 7                  # attention window
WORST = {"ratio": 0.0, "what": ""}          # largest |error| / bound of the real-data pass over the module


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    yield _lib
    print(f"\nreal-data pass: worst |error| / bound over all cases {WORST['ratio']:.3g} ({WORST['what']})")


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ================================================================================================ case tables
class Case:
    """One pk_wgrad_bf16 problem.  Linear form: Ho == 0, M rows; conv form: (B, Hs, Ws) -> (Ho, Wo) with M = B Ho Wo.
    maps: None, "win" (7x7 window partition of the (B, Hs, Ws) token grid, passed with the grid) or "any" (arbitrary map, no grid).
    launches: (n_bias, out_layout) of the launches with dw; the slab-only launch uses the first n_bias."""

    def __init__(self, name, kernel, tn, tc, mode, S, N, Cin, k=1, s=1, M=0, B=0, Hs=0, Ws=0, conv=False, flags=0, maps=None, rps=0,
                 launches=((0, 0),)):
        self.name, self.kernel, self.tn, self.tc, self.mode, self.S = name, kernel, tn, tc, mode, S
        self.N, self.Cin, self.k, self.s, self.B, self.Hs, self.Ws = N, Cin, k, s, B, Hs, Ws
        self.conv, self.flags, self.maps, self.rps, self.launches = conv, flags, maps, rps, launches
        self.T = k * k
        if conv:
            self.Ho, self.Wo = (Hs + 2 * (k // 2) - k) // s + 1, (Ws + 2 * (k // 2) - k) // s + 1
            self.M = B * self.Ho * self.Wo
        else:
            self.Ho = self.Wo = 0
            self.M = M
            if maps == "win":
                assert M == B * (-(-Hs // WS)) * (-(-Ws // WS)) * WS * WS

    def slices(self, L):
        return L.lib.pk_wgrad_slices(self.M, self.N, self.Cin, self.k, self.s, self.Hs, self.Ws, self.flags)

    def key(self):
        return (self.kernel, self.tn, self.tc, self.mode)


def _plain(name, tn, tc, S, N, Cin, **kw):          # k_wgrad4, no flags: dbias once with n_bias = N and once with n_bias < N
    return Case(name, "WGRAD4", tn, tc, 0, S, N, Cin, launches=((N, 1 if kw.get("conv") else 0), (N - 3, 0)), **kw)


def _conv3(name, kernel, tn, tc, S, B, Hs, Ws, Cin, N, s):          # 3x3: no bias path, both output layouts
    return Case(name, kernel, tn, tc, 0, S, N, Cin, k=3, s=s, B=B, Hs=Hs, Ws=Ws, conv=True, launches=((0, 0), (0, 1)))


CASES = [
    # plain k_wgrad4 (1x1 stride 1, linear layers)
    _plain("w4 64x64: S=9, last slice 257 rows, 7 padding workgroups", 64, 64, 9, 40, 24, M=4097),
    _plain("w4 64x128: last column tile 8 wide", 64, 128, 3, 64, 136, B=1, Hs=25, Ws=41, conv=True),
    _plain("w4 128x64: last n-tile 8 rows, bias there", 128, 64, 3, 136, 64, M=1025),
    _plain("w4 128x128", 128, 128, 3, 200, 264, B=5, Hs=5, Ws=41, conv=True),
    # column form: 3x3 stride 2, or stride 1 with Ws > 48
    _conv3("cols 64x128 stride 2: Cin=8, nine taps in one tile, odd 37x29", "WGRAD4_COLS", 64, 128, 3, 4, 37, 29, 8, 64, 2),
    _conv3("cols 128x128 stride 2: Cin=24, tile edge inside a tap", "WGRAD4_COLS", 128, 128, 2, 3, 32, 24, 24, 72, 2),
    _conv3("cols 64x128 stride 1: Ws=49, slices start mid-row, last tile 16 wide", "WGRAD4_COLS", 64, 128, 3, 2, 11, 49, 16, 32, 1),
    # nine-tap kernel
    _conv3("3x3 13x48: Ws at the halo limit, four tiles, S=5", "WGRAD4_3X3", 64, 64, 5, 3, 13, 48, 72, 72, 1),
    _conv3("3x3 40x2: advance wraps several rows per step", "WGRAD4_3X3", 64, 64, 1, 2, 40, 2, 8, 16, 1),
    _conv3("3x3 1x1: one-pixel maps", "WGRAD4_3X3", 64, 64, 1, 5, 1, 1, 8, 16, 1),
    # wide 3x3 kernel
    Case("w3: 91x91 256->256, S=9, ragged last slice", "WGRAD3", 256, 256, 0, 9, 256, 256, k=3, s=1, B=1, Hs=91, Ws=91, conv=True,
         launches=((0, 1),)),
    # k_wgrad2: 1x1 stride 2, and arbitrary row maps
    Case("w2 64: 1x1 stride 2, odd 35x27", "WGRAD2", 64, 64, 0, 3, 24, 40, k=1, s=2, B=3, Hs=35, Ws=27, conv=True, launches=((24, 1),)),
]
for _N, _C, _t in ((136, 128, 128), (40, 72, 64)):
    for _fl in (1, 2, 3, 7):
        CASES.append(Case(f"w2 {_t} flags {_fl}: arbitrary map", "WGRAD2", _t, _t, 0, 4, _N, _C, M=900, flags=_fl, maps="any", rps=100,
                          launches=((_N, 0),)))
# k_wgrad4w: every tile x mode, token grid 3 x 15 x 10 (pad tokens at the bottom and at the right), M = 882
for _N, _C, _tn, _tc in ((40, 24, 64, 64), (48, 136, 64, 128), (136, 56, 128, 64), (144, 200, 128, 128)):
    for _fl, _mode in ((1, 1), (6, 2), (4, 3), (2, 0), (7, 0)):
        CASES.append(Case(f"w4w {_tn}x{_tc} flags {_fl}: mode {_mode}", "WGRAD4W", _tn, _tc, _mode, 2, _N, _C, M=882, B=3, Hs=15, Ws=10,
                          flags=_fl, maps="win" if _fl & 3 else None, rps=150, launches=((_N, 0),)))
CASES.append(Case("w4w 64x64 flags 1 S=10: mode 1, grid 16 x 16 x 12", "WGRAD4W", 64, 64, 1, 10, 40, 24, M=4704, B=16, Hs=16, Ws=12, flags=1,
                  maps="win", launches=((40, 0),)))

# pk_wgrad_group members: (B, Hs, Ws, Cin, N, S)
GROUP_1X1 = [(1, 10, 10, 8, 8, 1), (1, 17, 241, 24, 40, 9), (1, 2, 3, 8, 16, 1), (5, 5, 41, 72, 136, 3), (1, 27, 19, 40, 24, 2),
             (1, 3, 683, 64, 72, 5), (1, 7, 7, 8, 64, 1), (2, 32, 24, 136, 8, 3), (31, 1, 1, 40, 40, 1), (3, 40, 25, 64, 64, 6),
             (1, 1, 1, 16, 8, 1), (1, 20, 32, 8, 200, 2)]
GROUP_3X3 = [(4, 37, 29, 8, 64, 3), (5, 63, 61, 24, 72, 10), (1, 5, 3, 8, 8, 1), (2, 9, 7, 16, 40, 1)]

ERR_INVALID, ERR_UNSUPPORTED = -1, -2


def test_case_tables_match_the_library():
    """No device is opened: S of every case is what the library's size queries return, and the cases cover every instantiation that
    pk_wgrad_bf16's switch and pk_wgrad_group launch (read from the source, so a new instantiation without a case fails here)."""
    from infantposeestimation_gaussianbias_amd import _lib as L
    for c in CASES:
        assert c.slices(L) == c.S, f"{c.name}: declared S = {c.S}, library {c.slices(L)}"
    for ks, st, members in ((1, 1, GROUP_1X1), (3, 2, GROUP_3X3)):
        for B, Hs, Ws, Cin, N, S in members:
            Ho, Wo = (Hs + 2 * (ks // 2) - ks) // st + 1, (Ws + 2 * (ks // 2) - ks) // st + 1
            got = L.lib.pk_wgrad_group_slices(B * Ho * Wo, N, Cin, ks, st)
            assert got == S, f"group member {(B, Hs, Ws, Cin, N)} k={ks}: declared S = {S}, library {got}"
    assert len(GROUP_1X1) == 12 and max(m[5] for m in GROUP_1X1) >= 9 and max(m[5] for m in GROUP_3X3) >= 9
    with open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "csrc", "pk_wgrad.hip")) as f:
        src = f.read()
    body = src[src.index('extern "C" int pk_wgrad_bf16'):]
    named = {(k, int(a), int(b), int(m)) for k, a, b, m in re.findall(r"WGRAD_CASE\(WG_(\w+), (\d+), (\d+), (\d+),", body)}
    named |= {(k, int(a), int(b), int(m)) for k, a, b, m in re.findall(r"case wgrad_key\(WG_(\w+), (\d+), (\d+), (\d+)\)", body)}
    named |= {("WGRAD4W", int(a), int(b), m) for a, b in re.findall(r"WGRAD4W_CASES\((\d+), (\d+)\)", body) for m in range(4)}
    assert len(named) == 26, sorted(named)
    assert {c.key() for c in CASES} == named, sorted(named ^ {c.key() for c in CASES})
    grouped = set(re.findall(r"k_wgrad4g<(\d+), (\d+), (\w+)>\)", src))
    assert grouped == {("64", "128", "true"), ("64", "64", "false")}, grouped          # GROUP_3X3 and GROUP_1X1 respectively


# ================================================================================================ data
def chan_data(rows, C, seed, offset):
    """bf16 [rows][C]: channel c ~ N(off_c, s_c^2), s_c = 10^U(-2, 2), |off_c| <= offset * s_c"""
    g = gen(seed)
    s = 10.0 ** (torch.rand(C, generator=g, device=DEV, dtype=F64) * 4 - 2)
    off = (torch.rand(C, generator=g, device=DEV, dtype=F64) * 2 - 1) * offset * s
    return (torch.randn(rows, C, generator=g, device=DEV, dtype=F32).double() * s + off).to(BF)


def int_data(rows, C, seed):
    """bf16 [rows][C] of small integers: even channels from {0..3}, odd channels from {-3..3}"""
    g = gen(seed)
    nonneg = torch.randint(0, 4, (rows, C), generator=g, device=DEV)
    signed = torch.randint(-3, 4, (rows, C), generator=g, device=DEV)
    return torch.where(torch.arange(C, device=DEV) % 2 == 0, nonneg, signed).to(BF)


def operand(rows, C, seed, exact, guard, offset, named=None):
    """-> (buffer, view): `rows` data rows between `guard` NaN rows on either side; rows outside `named` (if given) are NaN as well"""
    data = int_data(rows, C, seed) if exact else chan_data(rows, C, seed, offset)
    if named is not None:
        keep = torch.zeros(rows, dtype=torch.bool, device=DEV)
        keep[named] = True
        data[~keep] = NAN
    buf = torch.full((rows + 2 * guard, C), NAN, dtype=BF, device=DEV)
    buf[guard:guard + rows] = data
    return buf, buf[guard:guard + rows]


def row_scales(n, seed, exact):
    g = gen(seed)
    if exact:
        return torch.tensor([0.0, 0.5, 1.0, 2.0], device=DEV)[torch.randint(0, 4, (n,), generator=g, device=DEV)].contiguous()
    s = (10.0 ** (torch.rand(n, generator=g, device=DEV) * 2 - 1)).float()
    s[0] = 0.0
    if n > 1:
        s[1] = 1.0 / 0.9          # not exact in bf16 (nor in fp32): DropPath's 1 / keep_prob
    return s


def window_map(B, H, W):
    """int32 [B nh nw 49]: window-order token -> pixel row, -1 for the pad tokens at the bottom / right"""
    nh, nw = -(-H // WS), -(-W // WS)
    m = np.full((B, nh, nw, WS, WS), -1, dtype=np.int64)
    for wy in range(nh):
        for wx in range(nw):
            for ty in range(WS):
                for tx in range(WS):
                    y, x = wy * WS + ty, wx * WS + tx
                    if y < H and x < W:
                        m[:, wy, wx, ty, tx] = np.arange(B) * H * W + y * W + x
    return torch.from_numpy(m.reshape(-1).astype(np.int32)).to(DEV)


def any_map(M, src_rows, seed):
    """int32 [M]: a random selection, with repeats, from a random 60 % of the source rows, -1 at a random 10 % of the places"""
    g = gen(seed)
    pool = torch.randperm(src_rows, generator=g, device=DEV)[:src_rows * 6 // 10]
    m = pool[torch.randint(0, pool.numel(), (M,), generator=g, device=DEV)]
    m[torch.rand(M, generator=g, device=DEV) < 0.1] = -1
    return m.to(torch.int32).contiguous()


def taps(xv, B, Hs, Ws, Ho, Wo, k, s):
    """float64 [k*k][B Ho Wo][Cin]: the input pixel under every tap of every output pixel, zero outside the image (pad k // 2)"""
    p = k // 2
    x4 = xv.double().reshape(B, Hs, Ws, -1)
    xp = torch.zeros(B, Hs + 2 * p, Ws + 2 * p, x4.shape[-1], dtype=F64, device=DEV)
    xp[:, p:p + Hs, p:p + Ws] = x4
    return [xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s].reshape(B * Ho * Wo, -1) for kh in range(k) for kw in range(k)]


def gather(view, rowmap):
    """float64 rows of `view` through a map (-1 = zero row)"""
    if rowmap is None:
        return view.double()
    src = rowmap.long()
    rows = view[src.clamp_min(0)].double()
    return torch.where((src >= 0)[:, None], rows, torch.zeros_like(rows))


def scaled_rows(view, rowmap, scale, rps):
    """float64 G rows as the kernels multiply them: gathered, times scale[source row / rps] in fp32, re-rounded ONCE to bf16"""
    if scale is None:
        return gather(view, rowmap)
    src = torch.arange(view.shape[0], device=DEV) if rowmap is None else rowmap.long()
    ok = src >= 0
    src = src.clamp_min(0)
    rows = (view[src].float() * scale[src // rps][:, None]).to(BF).double()
    return torch.where(ok[:, None], rows, torch.zeros_like(rows))


def reference(G, X, want_abs):
    """G [M][N], X [T][M][Cin] float64 -> dw [N][T][Cin], dbias [N] (and the same of the absolute values, for the bound)"""
    dw = torch.stack([G.T @ x for x in X], 1)
    out = [dw, G.sum(0)]
    if want_abs:
        Ga = G.abs()
        out += [torch.stack([Ga.T @ x.abs() for x in X], 1), Ga.sum(0)]
    return out


# ================================================================================================ comparisons
def agree(got, ref, bound, what, exact):
    """exact pass: got == ref everywhere (a NaN fails); real pass: |got - ref| <= bound element-wise"""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if exact:
        bad = ~(got == ref)
        if bool(bad.any()):
            idx = bad.nonzero()
            i = tuple(int(v) for v in idx[0])
            raise AssertionError(f"{what}: {idx.shape[0]} of {got.numel()} differ from the exact result; first at {i}: got {float(got[i])!r}, "
                                 f"exact {float(ref[i])!r}; last at {tuple(int(v) for v in idx[-1])}")
        return
    d = (got - ref).abs()
    ratio = d / bound.clamp_min(1e-300)
    worst = float(ratio.nan_to_num(float("inf")).max()) if d.numel() else 0.0
    print(f"{what}: worst |error| / bound {worst:.3g}")
    if worst > WORST["ratio"]:
        WORST["ratio"], WORST["what"] = worst, what
    bad = ~(d <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(int(v) for v in idx[0])
        raise AssertionError(f"{what}: {idx.shape[0]} of {d.numel()} outside the bound; first at {i}: got {float(got[i])!r}, reference "
                             f"{float(ref[i])!r}, bound {float(bound[i])!r}; worst |error| / bound = {worst:.3g}")


def guarded(n, tail=1024):
    """fp32 buffer: n NaN, then `tail` sentinels"""
    t = torch.full((n + tail,), NAN, device=DEV)
    t[n:] = SENT
    return t


def intact(t, n, what):
    assert bool((t[n:] == SENT).all()), f"{what}: written past its {n} floats"


# ================================================================================================ pk_wgrad_bf16
def run_case(L, c, exact, seed):
    M, N, Cin, T, S = c.M, c.N, c.Cin, c.T, c.S
    tag = f"{c.name} [{'exact' if exact else 'real'}]"
    a_map = g_map = scale = None
    if c.conv:
        x_rows, g_rows, guard_x, guard_g = c.B * c.Hs * c.Ws, M, c.Hs * c.Ws, c.Ho * c.Wo
    else:
        x_rows = g_rows = M
        guard_x = guard_g = c.Hs * c.Ws if c.maps == "win" else 64
    x_named = g_named = None
    if c.maps == "win":
        wm = window_map(c.B, c.Hs, c.Ws)
        if c.flags & 1:
            a_map, x_rows = wm, c.B * c.Hs * c.Ws
        if c.flags & 2:
            g_map, g_rows = wm, c.B * c.Hs * c.Ws
    elif c.maps == "any":
        if c.flags & 1:
            x_rows = 1200
            a_map = any_map(M, x_rows, seed + 11)
            x_named = a_map[a_map >= 0].long()
        if c.flags & 2:
            g_rows = 1200
            g_map = any_map(M, g_rows, seed + 12)
            g_named = g_map[g_map >= 0].long()
    xbuf, xv = operand(x_rows, Cin, seed + 1, exact, guard_x, 8.0, x_named)
    gbuf, gv = operand(g_rows, N, seed + 2, exact, guard_g, 1.0, g_named)
    if c.flags & 4:
        scale = row_scales(-(-g_rows // c.rps), seed + 3, exact)
    G = scaled_rows(gv, g_map, scale, c.rps)
    X = taps(xv, c.B, c.Hs, c.Ws, c.Ho, c.Wo, c.k, c.s) if c.conv else [gather(xv, a_map)]
    assert G.shape == (M, N) and all(x.shape == (M, Cin) for x in X) and len(X) == T
    ref = reference(G, X, not exact)
    assert not bool(torch.isnan(ref[0]).any() or torch.isnan(ref[1]).any())
    bw, bb = (None, None) if exact else ((M + S + 16) * U * ref[2], (M + S + 16) * U * ref[3])
    total, ws_n = N * T * Cin, S * N * (T * Cin + 1)

    def launch(ws, dw, dbias, n_bias, layout):
        L.call("pk_wgrad_bf16", xv, gv, ws, dw, dbias, n_bias, a_map, g_map, scale, c.rps if scale is not None else 0, M, N, Cin, c.k, c.s,
               c.B, c.Hs, c.Ws, c.Ho, c.Wo, layout, L.stream_ptr())
        torch.cuda.synchronize()

    # slabs only: every slab element written, nothing beyond S N (T Cin + 1) floats, float64 slab sums = the result
    n_bias = c.launches[0][0]
    ws = guarded(ws_n)
    launch(ws, None, None, n_bias, 0)
    intact(ws, ws_n, f"{tag}: workspace (slabs only)")
    wslab, bslab = ws[:S * total].reshape(S, N, T, Cin), ws[S * total:ws_n].reshape(S, N)
    assert not bool(torch.isnan(wslab).any()), f"{tag}: {int(torch.isnan(wslab).sum())} weight-slab elements unwritten or NaN"
    agree(wslab.double().sum(0), ref[0], bw, f"{tag}: float64 sum of the weight slabs", exact)
    if n_bias:
        assert not bool(torch.isnan(bslab).any()), f"{tag}: {int(torch.isnan(bslab).sum())} bias-slab elements unwritten or NaN"
        agree(bslab.double().sum(0), ref[1], bb, f"{tag}: float64 sum of the bias slabs", exact)
    else:
        assert bool(torch.isnan(bslab).all()), f"{tag}: bias slabs written without n_bias"
    # reduced outputs
    for n_bias, layout in c.launches:
        ws, dw, db = guarded(ws_n), guarded(total, 64), guarded(n_bias, 8)
        launch(ws, dw, db if n_bias else None, n_bias, layout)
        intact(ws, ws_n, f"{tag}: workspace")
        intact(dw, total, f"{tag}: dw")
        intact(db, n_bias, f"{tag}: dbias (n_bias {n_bias} of {N})")
        want = ref[0].permute(0, 2, 1) if layout == 1 else ref[0]
        bnd = None if exact else (bw.permute(0, 2, 1) if layout == 1 else bw)
        agree(dw[:total].reshape(want.shape), want, bnd, f"{tag}: dw (layout {layout})", exact)
        if n_bias:
            agree(db[:n_bias], ref[1][:n_bias], None if exact else bb[:n_bias], f"{tag}: dbias (n_bias {n_bias} of {N})", exact)
    del xbuf, gbuf


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name.split(":")[0] for c in CASES])
def test_wgrad_exact_then_real_with_guards(L, case):
    assert case.slices(L) == case.S
    seed = 1000 * CASES.index(case)
    run_case(L, case, True, seed)
    run_case(L, case, False, seed + 500)


# ================================================================================================ pk_wgrad_group
def run_group(L, ks, st, members, exact, seed):
    from infantposeestimation_gaussianbias_amd import exchange
    rows, keep = [], []
    for i, (B, Hs, Ws, Cin, N, S) in enumerate(members):
        Ho, Wo = (Hs + 2 * (ks // 2) - ks) // st + 1, (Ws + 2 * (ks // 2) - ks) // st + 1
        xbuf, xv = operand(B * Hs * Ws, Cin, seed + 10 * i + 1, exact, Hs * Ws, 8.0)
        gbuf, gv = operand(B * Ho * Wo, N, seed + 10 * i + 2, exact, Ho * Wo, 1.0)
        total = N * ks * ks * Cin
        ws = guarded(S * total)
        rows.append(dict(x=xv.data_ptr(), grad_out=gv.data_ptr(), workspace=ws.data_ptr(), B=B, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, N=N, Cin=Cin, ksize=ks,
                         stride=st))
        keep.append((xbuf, xv, gbuf, gv, ws, Ho, Wo, total))
    exchange._launch("pk_wgrad_group", exchange.WG_DT, rows)
    torch.cuda.synchronize()
    for i, (B, Hs, Ws, Cin, N, S) in enumerate(members):
        xbuf, xv, gbuf, gv, ws, Ho, Wo, total = keep[i]
        M = B * Ho * Wo
        tag = f"group k={ks} member {i} {(B, Hs, Ws, Cin, N)} S={S} [{'exact' if exact else 'real'}]"
        ref = reference(gv.double(), taps(xv, B, Hs, Ws, Ho, Wo, ks, st), not exact)
        intact(ws, S * total, f"{tag}: workspace")
        slab = ws[:S * total].reshape(S, N, ks * ks, Cin)
        assert not bool(torch.isnan(slab).any()), f"{tag}: {int(torch.isnan(slab).sum())} slab elements unwritten or NaN"
        agree(slab.double().sum(0), ref[0], None if exact else (M + S + 16) * U * ref[2], f"{tag}: float64 sum of the slabs", exact)


@gpu
@pytest.mark.parametrize("ks,st,members", [(1, 1, GROUP_1X1), (3, 2, GROUP_3X3)], ids=["1x1 stride 1", "3x3 stride 2"])
def test_wgrad_group_members_exact_then_real(L, ks, st, members):
    for B, Hs, Ws, Cin, N, S in members:
        Ho, Wo = (Hs + 2 * (ks // 2) - ks) // st + 1, (Ws + 2 * (ks // 2) - ks) // st + 1
        assert L.lib.pk_wgrad_group_slices(B * Ho * Wo, N, Cin, ks, st) == S
    run_group(L, ks, st, members, True, 70000 + ks)
    run_group(L, ks, st, members, False, 80000 + ks)


# ================================================================================================ argument checks
@gpu
def test_wgrad_argument_checks_launch_nothing(L):
    """Refused calls on real tensors: the stated error code, no launch, no fault, outputs untouched."""
    from infantposeestimation_gaussianbias_amd import exchange
    x = torch.ones(4096, 64, dtype=BF, device=DEV)
    g = torch.ones(4096, 64, dtype=BF, device=DEV)
    ws, dw, db = (torch.full((1 << 20,), SENT, device=DEV) for _ in range(3))
    rowmap = torch.zeros(4096, dtype=torch.int32, device=DEV)
    scale = torch.ones(64, device=DEV)
    st = L.stream_ptr()
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def single(n_bias=0, a_map=None, g_map=None, g_scale=None, rps=0, M=512, N=32, Cin=32, k=1, s=1, B=0, Hs=0, Ws=0, Ho=0, Wo=0, dbias=None):
        return L.lib.pk_wgrad_bf16(p(x), p(g), p(ws), p(dw), p(dbias), n_bias, p(a_map), p(g_map), p(g_scale), rps, M, N, Cin, k, s, B, Hs, Ws,
                                   Ho, Wo, 0, st)

    def group(members):
        arr = np.zeros(len(members), dtype=exchange.WG_DT)
        for i, (B, Hs, Ws, Cin, N, ks, s_) in enumerate(members):
            Ho, Wo = (Hs + 2 * (ks // 2) - ks) // s_ + 1, (Ws + 2 * (ks // 2) - ks) // s_ + 1
            for k_, v in dict(x=p(x), grad_out=p(g), workspace=p(ws), B=B, Hs=Hs, Ws=Ws, Ho=Ho, Wo=Wo, N=N, Cin=Cin, ksize=ks, stride=s_).items():
                arr[i][k_] = v
        return L.lib.pk_wgrad_group(arr.ctypes.data, len(members), st)

    conv = dict(M=2 * 16 * 12, B=2, Hs=16, Ws=12, Ho=16, Wo=12)
    assert single(**conv) == 0 and single(M=392, B=2, Hs=9, Ws=10, a_map=rowmap) == 0        # the accepted twins of the refused calls below
    assert group([(2, 16, 12, 32, 32, 1, 1)]) == 0 and group([(2, 16, 12, 32, 32, 3, 2)] * 12) == 0
    torch.cuda.synchronize()
    ws.fill_(SENT)
    dw.fill_(SENT)
    checks = [
        ("n_bias > N", ERR_INVALID, lambda: single(n_bias=33, dbias=db)),
        ("a_rowmap with the conv form", ERR_INVALID, lambda: single(a_map=rowmap, **conv)),
        ("g_rowmap with the conv form", ERR_INVALID, lambda: single(g_map=rowmap, **conv)),
        ("M is not the window-order count of the grid", ERR_INVALID, lambda: single(M=391, B=2, Hs=9, Ws=10, a_map=rowmap)),
        ("M is not the window-order count of the grid (g_map + g_scale)", ERR_INVALID,
         lambda: single(M=441, B=2, Hs=9, Ws=10, g_map=rowmap, g_scale=scale, rps=90)),
        ("thirteen members", ERR_INVALID, lambda: group([(2, 16, 12, 32, 32, 1, 1)] * 13)),
        ("mixed kinds", ERR_INVALID, lambda: group([(2, 16, 12, 32, 32, 1, 1), (2, 16, 12, 32, 32, 3, 2)])),
        ("mixed kinds, 3x3 first", ERR_INVALID, lambda: group([(2, 16, 12, 32, 32, 3, 2), (2, 16, 12, 32, 32, 1, 1)])),
        ("group of 3x3 stride 1", ERR_UNSUPPORTED, lambda: group([(2, 16, 12, 32, 32, 3, 1)] * 2)),
        ("Cin not a multiple of 8", ERR_UNSUPPORTED, lambda: single(Cin=36)),
        ("N not a multiple of 8", ERR_UNSUPPORTED, lambda: single(N=36)),
        ("group: Cin not a multiple of 8", ERR_UNSUPPORTED, lambda: group([(2, 16, 12, 36, 32, 1, 1)])),
        ("group: N not a multiple of 8", ERR_UNSUPPORTED, lambda: group([(2, 16, 12, 32, 36, 3, 2)])),
        ("dbias on the nine-tap route", ERR_UNSUPPORTED, lambda: single(n_bias=32, dbias=db, k=3, **conv)),
        ("dbias on the column-form route", ERR_UNSUPPORTED,
         lambda: single(n_bias=32, dbias=db, k=3, s=2, M=2 * 8 * 6, B=2, Hs=16, Ws=12, Ho=8, Wo=6)),
    ]
    for what, code, fn in checks:
        rc = fn()
        assert rc == code, f"{what}: returned {rc}, expected {code} ({L.lib.pk_last_error_string().decode()})"
    torch.cuda.synchronize()
    for name, t in (("workspace", ws), ("dw", dw), ("dbias", db)):
        assert bool((t == SENT).all()), f"a refused call wrote to {name}"
