"""Every forward / data-gradient kernel of csrc/pk_igemm.hip where its tiles end, against float64.

Which kernel, tile and grid a contraction gets follows from its shape, its options and the alignment of its pointers alone (igemm_route),
so every case below is a problem chosen for the instantiation it selects and the edge it puts inside it.  Each case DECLARES its route in
the words of tests/launch_recorder.hip (kernel and template arguments, grid, the launcher-set flags v8 / cm / dg, the statistics rows);
test_case_tables_match_the_library (no device needed) feeds every case to the recorder's case mode, holds the declaration against what the
real entry points launch, and holds the set of instantiations the cases reach against IGEMM_TILES, IGEMM_GROUP_TILES and the CONV3H_CASE
list of the source: a new instantiation without a case fails there by name.  Entries are called through the C-ABI; packed weights are
built here with torch ([Cout][k*k][Cin]; data gradients in the flipped form dst[c][T-1-t][n] = src[n][c][t] of the header).

Two passes per case, both against a float64 reference assembled from strided slices of the zero-padded input, one matmul per tap (no index
arithmetic shared with the kernels); the dilated form is the header's definition: the input zero-stuffed to (Ho, Wo), then a stride-1
contraction with the packed weights.
  * exact: x holds small integers (even channels {0..3}, odd {-3..3}), w integers of {-2..2} with half of them zero, bias multiples of
    0.5, col_scale from {-1, 0.5, 1, 2}, res_scale from {0, 0.5, 1, 2}, integer residuals.  The test asserts ON THE REFERENCE (before any
    launch; test_exact_operands_stay_below_2_24 does it without a device) that sum |a||w| of every output and sum |v|, sum v^2 of every
    128-row statistics tile stay below 2^24: every fp32 sum is then exact in any order, and fp32 outputs, every statistics row of the
    tile and ring kernels (rows are defined per 128 output pixels; the halo kernel's rows are per workgroup: their float64 sum),
    preact_out and -- f32_to_bf16 being round-to-nearest-even -- bf16 outputs must EQUAL the reference (rounded once to bf16).  Only
    values behind GELU, gelu' and softplus are held to a bound instead; their pre-activation is held exactly through preact_out or a
    twin launch without the activation.
  * real: bf16 data with a per-channel scale spread over 10^-2 .. 10^2, row scales including 0 and 1/0.9.  With U = 2^-24, per element:
      accumulator         E = (T Cin + 16) U sum |a||w|               (T Cin non-zero fp32 additions in any order, 16 for the MFMA's own)
      each epilogue step  carries the incoming error times the factor it applies and adds 8 U (sum of the magnitudes of its terms)
      bf16 store          + half an ulp of |ref| + error so far: 2^(floor(log2 .) - 8), which lies between 2^-9 and 2^-8 of that magnitude
                          (2^-9 relative is the half-ulp just BELOW a power of two only: 1 + 2^-8 rounds to 1 or 1 + 2^-7, 2^-8 away, so a
                          flat 2^-9 (|ref| + E) would fail a correct round-to-nearest store; the exact half-ulp is the tightest true bound)
      statistics row      sum:  sum_rows E + (128 + 16) U sum_rows (|v| + E)
                          sum of squares:  sum_rows (2 |v| E + E^2) + (128 + 17) U sum_rows (|v| + E)^2
                          (the errors of the 128 accumulators, plus 128 fp32 additions in any order and the lane combine; one rounding per
                          square.  The float64 sum of rows is held to the sum of the row bounds; the halo kernel's rows hold up to M
                          pixels, so M takes the place of 128 there.)
    All of it is derived, none measured.  The module-level worst |error| / bound is printed at the end, apart for bf16 stores and for fp32
    results.  On MI355X: fp32 outputs 0.018, statistics 0.008 (worst-case bounds: the errors of K additions do not line up), bf16 stores
    1.0 -- a store's bound is its half-ulp plus a far smaller accumulator term, and among a million stores some land on a rounding tie.
  * transcendental epilogues: the activation's own error is a term ACT_TERM[name] (1 + |ref|), set to four times the worst value measured
    against float64 over EVERY finite bf16 pre-activation of magnitude <= 32 (test_activation_error_is_measured: identity weights make the
    fp32 pre-activation the bf16 input itself).  Measured on MI355X: GELU 2.11e-7, gelu' 1.59e-7, softplus 8.45e-8.  The term may not pass
    2^-16, 1/128 of the bf16 half-ulp; the test asserts both.

Guards, both passes: x, w, residual, gelu_grad_of are views into larger buffers with at least one sample's worth of NaN before and after;
rows a row map never names are NaN.  Outputs, preact_out and the statistics buffer (pk_conv_stats_rows rows, not more) are NaN up to their
documented size and followed, inside the same allocation, by a sentinel region of at least one full row and never below 4096 elements.
Every documented element must be written and no sentinel touched; output rows an o_rowmap never names keep their prefill; every launch
runs twice and must be bit-identical.

Not covered: M >= 2^24 (the exact-division path of `idiv`) needs tensors far beyond a test of a few seconds.  The route of the 256 x 128
tile asks for N % 128 == 0, so that tile has no ragged last column tile to test; every other tile instantiation has one.
"""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
LIMIT = float(2 ** 24)
NAN = float("nan")
SENT = 24576.0            # sentinel value (exact in bf16 and fp32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}          # kind -> (largest |error| / bound of the bounded comparisons over the module, where)
# activation error relative to (1 + |ref|): four times the worst value measured by test_activation_error_is_measured (see the docstring)
ACT_TERM = {"gelu": 4 * 2.11e-7, "gelu_grad": 4 * 1.59e-7, "softplus": 4 * 8.45e-8}
ACT_CAP = 2.0 ** -16
ACT_SEEN = {}
GELU_LIP = 1.13           # max |gelu'|


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    yield _lib
    print()
    for kind, (ratio, what) in sorted(WORST.items()):
        print(f"bounded comparisons, {kind}: worst |error| / bound over all cases {ratio:.3g} ({what})")
    for k, v in ACT_SEEN.items():
        print(f"activation error of {k}: worst |error| / (1 + |ref|) = {v:.3g} (term {ACT_TERM[k]:.3g}, cap {ACT_CAP:.3g})")


# ================================================================================================ case tables
EDGES = ("ragged M", "ragged N", "N%8==4", "K tail", "G%8==0", "G%8!=0", "sample boundary", "parity boundary")


def _edges(text):
    got = tuple(e.strip() for e in text.split(",") if e.strip())
    assert all(e in EDGES for e in got), got
    return got


class Conv:
    """One pk_conv2d_nhwc (entry "conv") or pk_conv2d_affine_nhwc (entry "affine") problem in the kernel's own terms: x (B, Hs, Ws, Cin) ->
    out (B, Ho, Wo, Cout); d = 1 is the dilated form (Ho, Wo given: 2 Hs - 1 or 2 Hs).  st: statistics; ad / re: addend / residual (2: its
    pointer 8 bytes off a 16-byte boundary); bi: bias; act: 2 softplus; om: out_mode; sc 2: col_scale / shift 4 bytes off; sw: routing
    switches (1: both specialised kernels from one tile on).  route: the declaration, in the recorder's words."""
    kind = "conv"

    def __init__(self, name, route, edges, B, Hs, Ws, Cin, Cout, k, s=1, d=0, Ho=0, Wo=0, st=0, ad=0, bi=0, act=0, om=0, entry="conv", re=0, sc=1,
                 relu=0, sw=0):
        self.name, self.route, self.edges = name, route, _edges(edges)
        self.B, self.Hs, self.Ws, self.Cin, self.Cout, self.k, self.s, self.d = B, Hs, Ws, Cin, Cout, k, s, d
        if not d:
            Ho, Wo = (Hs + 2 * (k // 2) - k) // s + 1, (Ws + 2 * (k // 2) - k) // s + 1
        self.Ho, self.Wo, self.M, self.T = Ho, Wo, B * Ho * Wo, k * k
        self.st, self.ad, self.bi, self.act, self.om, self.entry, self.re, self.sc, self.relu, self.sw = st, ad, bi, act, om, entry, re, sc, relu, sw

    def line(self):
        geo = f"B={self.B} {self.Hs}x{self.Ws} ci={self.Cin} co={self.Cout} k={self.k} s={self.s}"
        if self.entry == "affine":
            return f"affine {geo} re={self.re} sc={self.sc} relu={self.relu} oa=0"
        return f"conv {geo} d={self.d} st={self.st} ad={self.ad} bi={self.bi} act={self.act} om={self.om} oa=0 Ho={self.Ho} Wo={self.Wo}"


class Lin:
    """One pk_linear_bf16 problem.  maps: 2 a_rowmap, 3 o_rowmap (both with -1 rows); pg: 1 preact_out, 2 gelu_grad_of, 3 preact_out 8 bytes
    off a 16-byte boundary; act 1: GELU; f32: fp32 output; re: residual with res_scale, rps rows per sample."""
    kind = "linear"
    sw = 0

    def __init__(self, name, route, edges, M, N, K, maps=0, pg=0, act=0, f32=0, re=0, rps=0):
        self.name, self.route, self.edges = name, route, _edges(edges)
        self.M, self.N, self.K, self.maps, self.pg, self.act, self.f32, self.re, self.rps = M, N, K, maps, pg, act, f32, re, rps
        self.T, self.Cin = 1, K

    def line(self):
        return f"linear M={self.M} N={self.N} K={self.K} maps={self.maps} pg={self.pg} act={self.act} f32={self.f32} re={self.re} rps={self.rps}"


class Group:
    """One pk_conv2d_group launch.  members: Conv objects (entry "conv": statistics or addend; entry "affine": scale / shift / residual / ReLU)."""
    kind = "cgroup"
    sw = 0

    def __init__(self, name, route, edges, members):
        self.name, self.route, self.edges, self.members = name, route, _edges(edges), members

    def line(self):
        ms = []
        for m in self.members:
            aff = m.entry == "affine"
            ms.append("m=" + ",".join(str(v) for v in (m.B, m.Hs, m.Ws, m.Cin, m.Cout, m.k, m.s, m.d, m.Ho, m.Wo, m.st, 1 if aff else 0,
                                                        m.re if aff else m.ad, 3 if aff and m.relu else 0)))
        return f"cgroup n={len(self.members)} " + " ".join(ms)


def _dgrad(Hs, Ws, odd):
    """output size of the dilated form: odd -> (2 Hs - 1, 2 Ws - 1), the four parity classes differ in size"""
    return dict(d=1, Ho=2 * Hs - (1 if odd else 0), Wo=2 * Ws - (1 if odd else 0))


CONVS = [
    # ---- 256 x 128 tile (N % 128 == 0, T Cin >= 576, >= 1024 workgroups; Cout % 256 != 0 keeps the default switches off the ring kernel)
    Conv("t256 L3 stats bf16: M % 256 = 57, second statistics group of the last tile beyond M", "k_igemm2<256,128,2,2,32,3> g=115,9 v8=1 cm=0 dg=0 rows=229",
         "ragged M, G%8!=0", 1, 171, 171, 64, 1152, 3, st=1),
    Conv("t256 L3 stats fp32: M % 256 = 125, G % 8 == 0", "k_igemm2<256,128,2,2,32,3> g=120,9 v8=1 cm=0 dg=0 rows=239",
         "ragged M, G%8==0", 1, 169, 181, 64, 1152, 3, st=1, om=1),
    Conv("t256 L4: stride-2 data gradient, odd 171 x 171, tiles straddle parity classes", "k_igemm2<256,128,2,2,32,4> g=115,9 v8=1 cm=0 dg=1 rows=229",
         "ragged M, G%8!=0, parity boundary", 1, 86, 86, 64, 1152, 3, **_dgrad(86, 86, True)),
    # ---- 128 x 128 tile, LEAN 4 (stride-2 data gradients wide enough for >= 512 workgroups)
    Conv("t128x128 L4 BK32: even 96 x 90, last column tile 8 wide", "k_igemm2<128,128,2,2,32,4> g=68,9 v8=1 cm=0 dg=1 rows=68",
         "ragged M, ragged N, G%8!=0, parity boundary", 1, 48, 45, 32, 1032, 3, **_dgrad(48, 45, False)),
    Conv("t128x128 L4 BK64: odd 93 x 89, addend", "k_igemm2<128,128,2,2,64,4> g=65,9 v8=1 cm=0 dg=1 rows=65",
         "ragged M, ragged N, G%8!=0, parity boundary", 1, 47, 45, 64, 1032, 3, ad=1, **_dgrad(47, 45, True)),
    # ---- 128 x 128 tile, LEAN 3 (statistics with N > 64 and T Cin > 256)
    Conv("t128x128 L3 BK32 stats: Cin 40 K tail, N 136", "k_igemm2<128,128,2,2,32,3> g=2,2 v8=1 cm=0 dg=0 rows=2",
         "ragged M, ragged N, K tail, sample boundary, G%8!=0", 2, 9, 11, 40, 136, 3, st=1),
    Conv("t128x128 L3 BK32 stats: Cin 72 K tail, stride 2, one ragged tile", "k_igemm2<128,128,2,2,32,3> g=1,2 v8=1 cm=0 dg=0 rows=1",
         "ragged M, ragged N, K tail, sample boundary", 2, 13, 11, 72, 136, 3, s=2, st=1),
    Conv("t128x128 L3 BK64 stats: N 136, fp32 output", "k_igemm2<128,128,2,2,64,3> g=2,2 v8=1 cm=0 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 3, 7, 9, 64, 136, 3, st=1, om=1),
    Conv("t128x128 L3 BK32 no stats: N 1024, M 8100", "k_igemm2<128,128,2,2,32,3> g=64,8 v8=1 cm=0 dg=0 rows=64",
         "ragged M, G%8==0", 1, 90, 90, 32, 1024, 3),
    # ---- 128 x 64 and 128 x 32 tiles, LEAN 3
    Conv("t128x64 L3 BK32 stats: 3x3 Cin 24 N 56", "k_igemm2<128,64,4,1,32,3> g=3,1 v8=1 cm=0 dg=0 rows=3",
         "ragged M, ragged N, K tail, sample boundary", 2, 11, 13, 24, 56, 3, st=1),
    Conv("t128x64 L3 BK64: 1x1 stride 2 Cin 192 N 40, addend 8 bytes off", "k_igemm2<128,64,4,1,64,3> g=2,1 v8=0 cm=0 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 5, 15, 9, 192, 40, 1, s=2, ad=2),
    Conv("t128x64 L3 BK32 stats: 1x1 Cin 40 N 76, scalar epilogue", "k_igemm2<128,64,4,1,32,3> g=2,2 v8=0 cm=0 dg=0 rows=2",
         "ragged M, ragged N, N%8==4, K tail, sample boundary", 2, 9, 8, 40, 76, 1, st=1),
    Conv("t128x32 L3 BK32 stats: 3x3 stride 2 Cin 8 N 20, maps 3 wide", "k_igemm2<128,32,4,1,32,3> g=3,1 v8=0 cm=0 dg=0 rows=3",
         "ragged M, ragged N, N%8==4, K tail, sample boundary", 30, 9, 3, 8, 20, 3, s=2, st=1),
    Conv("t128x32 L3 BK64 chunk-major: Cin 128 N 24", "k_igemm2<128,32,4,1,64,3> g=2,1 v8=1 cm=1 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 2, 10, 9, 128, 24, 3),
    Conv("t128x32 L3 BK64 chunk-major: Cin 192 N 8, maps 1 wide", "k_igemm2<128,32,4,1,64,3> g=2,1 v8=1 cm=1 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 3, 50, 1, 192, 8, 3, st=1),
    Conv("t128x32 L3 BK64: Cin 64 N 72 on few rows, maps 2 wide", "k_igemm2<128,32,4,1,64,3> g=3,3 v8=1 cm=0 dg=0 rows=3",
         "ragged M, ragged N, sample boundary", 4, 35, 2, 64, 72, 3),
    # ---- 128 x 64 and 128 x 32 tiles, LEAN 4
    Conv("t128x64 L4 BK32: 3x3 odd 9 x 13, addend, a tile spans all classes", "k_igemm2<128,64,4,1,32,4> g=2,1 v8=1 cm=0 dg=1 rows=2",
         "ragged M, ragged N, K tail, parity boundary", 2, 5, 7, 24, 40, 3, ad=1, **_dgrad(5, 7, True)),
    Conv("t128x64 L4 BK64: dilated 1x1 (T = 1) Cin 192 N 56", "k_igemm2<128,64,4,1,64,4> g=2,1 v8=1 cm=0 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 2, 6, 5, 192, 56, 1, **_dgrad(6, 5, False)),
    Conv("t128x32 L4 BK32: Ho = 1, two parity classes empty, N 20", "k_igemm2<128,32,4,1,32,4> g=3,1 v8=0 cm=0 dg=1 rows=3",
         "ragged M, ragged N, N%8==4, K tail, parity boundary", 40, 1, 4, 40, 20, 3, d=1, Ho=1, Wo=8),
    Conv("t128x32 L4 BK32: Wo = 1 with statistics (no parity grouping)", "k_igemm2<128,32,4,1,32,4> g=2,1 v8=1 cm=0 dg=0 rows=2",
         "ragged M, ragged N, K tail, sample boundary", 20, 5, 1, 8, 8, 3, st=1, d=1, Ho=9, Wo=1),
    Conv("t128x32 L4 BK32: one tile holds all four classes", "k_igemm2<128,32,4,1,32,4> g=1,1 v8=1 cm=0 dg=1 rows=1",
         "ragged M, ragged N, K tail, parity boundary", 1, 5, 4, 8, 8, 3, d=1, Ho=9, Wo=8),
    Conv("t128x32 L4 BK64: 32 x 24, whole tiles in one class (1, 2, 2, 4 taps)", "k_igemm2<128,32,4,1,64,4> g=18,1 v8=1 cm=0 dg=1 rows=18",
         "ragged N, parity boundary, G%8!=0", 3, 16, 12, 64, 24, 3, **_dgrad(16, 12, False)),
    Conv("t128x32 L4 BK64: odd 13 x 9, ragged rows", "k_igemm2<128,32,4,1,64,4> g=2,1 v8=1 cm=0 dg=1 rows=2",
         "ragged M, ragged N, parity boundary", 2, 7, 5, 64, 24, 3, **_dgrad(7, 5, True)),
    # ---- head outputs: fp32 NCHW planes with bias and softplus; fp32 rows with bias
    Conv("head planes: 1x1 Cout 17, softplus, tiles cross samples", "k_igemm2<128,32,4,1,32,3> g=2,1 v8=0 cm=0 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 3, 9, 7, 32, 17, 1, bi=1, act=2, om=2),
    Conv("head planes: 3x3 Cout 34, softplus", "k_igemm2<128,64,4,1,64,3> g=2,1 v8=0 cm=0 dg=0 rows=2",
         "ragged M, ragged N, sample boundary", 2, 11, 9, 64, 34, 3, bi=1, act=2, om=2),
    Conv("fp32 rows with bias: 3x3 Cin 16 N 40", "k_igemm2<128,64,4,1,32,3> g=2,1 v8=1 cm=0 dg=0 rows=2",
         "ragged M, ragged N, K tail, sample boundary", 2, 9, 11, 16, 40, 3, bi=1, om=1),
    # ---- pk_conv2d_affine_nhwc
    Conv("affine tile: 3x3 stride 2, scale shift residual ReLU", "k_igemm2<128,64,4,1,32,3> g=1,1 v8=1 cm=0 dg=0",
         "ragged M, ragged N, sample boundary", 3, 13, 10, 32, 48, 3, s=2, entry="affine", re=1, relu=1),
    Conv("affine ring: scale shift ReLU (the ring kernel takes no residual), M % 256 = 67", "k_conv8p g=2,1 v8=1 cm=0 dg=0",
         "ragged M", 1, 17, 19, 64, 256, 3, entry="affine", relu=1, sw=1),
    Conv("affine halo: scale shift residual ReLU", "k_conv3h<64,64> g=4,1 v8=1 cm=0 dg=0",
         "ragged M, sample boundary", 2, 11, 13, 64, 64, 3, entry="affine", re=1, relu=1, sw=1),
    Conv("affine, col_scale 4 bytes off: the ring shape goes back to the tile family", "k_igemm2<128,32,4,1,64,3> g=3,8 v8=1 cm=0 dg=0",
         "ragged M, G%8==0", 1, 17, 19, 64, 256, 3, entry="affine", sc=2, relu=1, sw=1),
    Conv("affine, residual on the ring shape: tile family", "k_igemm2<128,32,4,1,64,3> g=3,8 v8=1 cm=0 dg=0",
         "ragged M, G%8==0", 1, 17, 19, 64, 256, 3, entry="affine", re=1, relu=1, sw=1),
    # ---- ring kernel k_conv8p (forward with statistics, data gradient = the same contraction without them; an addend leaves the kernel)
    Conv("ring stats: a tile of 20 live rows", "k_conv8p g=1,1 v8=1 cm=0 dg=0 rows=1", "ragged M", 1, 5, 4, 256, 256, 3, st=1, sw=1),
    Conv("ring stats: M % 256 = 67", "k_conv8p g=2,1 v8=1 cm=0 dg=0 rows=3", "ragged M", 1, 17, 19, 64, 256, 3, st=1, sw=1),
    Conv("ring data gradient: two n-tiles, M % 256 = 41", "k_conv8p g=4,1 v8=1 cm=0 dg=0 rows=3", "ragged M", 1, 33, 9, 128, 512, 3, sw=1),
    Conv("ring shape with addend: tile family", "k_igemm2<128,32,4,1,64,3> g=3,8 v8=1 cm=0 dg=0 rows=3", "ragged M, G%8==0", 1, 17, 19, 64, 256, 3,
         ad=1, sw=1),
    # ---- halo kernel k_conv3h, every channel combination
    Conv("halo 32->32 stats: 9 x 7", "k_conv3h<32,32> g=2,1 v8=1 cm=0 dg=0 rows=4", "ragged M, sample boundary", 2, 9, 7, 32, 32, 3, st=1, sw=1),
    Conv("halo 64->64 stats: map 100 wide", "k_conv3h<64,64> g=34,1 v8=1 cm=0 dg=0 rows=68", "ragged M", 1, 40, 100, 64, 64, 3, st=1, sw=1),
    Conv("halo 64->32 data gradient: 5 x 5", "k_conv3h<64,32> g=1,1 v8=1 cm=0 dg=0 rows=2", "ragged M", 1, 5, 5, 64, 32, 3, sw=1),
    Conv("halo 32->64 data gradient with addend: 7 x 30", "k_conv3h<32,64> g=12,1 v8=1 cm=0 dg=0 rows=24", "ragged M, sample boundary", 5, 7, 30, 32, 64, 3,
         ad=1, sw=1),
    Conv("halo 32->32 stats: 70 maps of 3 x 3", "k_conv3h<32,32> g=14,1 v8=1 cm=0 dg=0 rows=28", "ragged M, sample boundary", 70, 3, 3, 32, 32, 3,
         st=1, sw=1),
]

LINS = [
    # ---- the lean instantiations (K % 64 == 0, K > 128, bf16 output, 16-byte aligned pointers)
    Lin("lin L1 128x64: plain, M 300", "k_igemm2<128,64,4,1,64,1> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 56, 192),
    Lin("lin L1 128x64: a_rowmap, K 320", "k_igemm2<128,64,4,1,64,1> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 56, 320, maps=2),
    Lin("lin L1 128x64: N 136, M 21 800", "k_igemm2<128,64,4,1,64,1> g=171,3 v8=1 cm=0 dg=0", "ragged M, ragged N, G%8!=0", 21800, 136, 192),
    Lin("lin L2 128x64: preact + GELU, one row in the last tile", "k_igemm2<128,64,4,1,64,2> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 257, 56, 320,
        pg=1, act=1),
    Lin("lin L2 128x64: gelu_grad_of", "k_igemm2<128,64,4,1,64,2> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 56, 192, pg=2),
    Lin("lin L1 128x32: o_rowmap, residual, res_scale, 49 rows per sample", "k_igemm2<128,32,4,1,64,1> g=3,3 v8=1 cm=0 dg=0",
        "ragged M, ragged N, sample boundary", 300, 72, 192, maps=3, re=1, rps=49),
    Lin("lin L1 128x32: plain, one row in the last tile", "k_igemm2<128,32,4,1,64,1> g=3,3 v8=1 cm=0 dg=0", "ragged M, ragged N", 257, 72, 320),
    Lin("lin L2 128x32: preact + GELU", "k_igemm2<128,32,4,1,64,2> g=3,3 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 72, 320, pg=1, act=1),
    Lin("lin L2 128x32: gelu_grad_of, a_rowmap", "k_igemm2<128,32,4,1,64,2> g=3,3 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 72, 192, maps=2, pg=2),
    # ---- what leaves them
    Lin("lin fp32 output: LEAN 3 of the 128x64 tile", "k_igemm2<128,64,4,1,64,3> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 56, 192, f32=1),
    Lin("lin preact_out 8 bytes off: LEAN 3, scalar preact", "k_igemm2<128,64,4,1,64,3> g=3,1 v8=0 cm=0 dg=0", "ragged M, ragged N", 300, 56, 192,
        pg=3, act=1),
    Lin("lin K 32: fp32 GELU", "k_igemm2<128,64,4,1,32,3> g=3,1 v8=1 cm=0 dg=0", "ragged M, ragged N", 300, 40, 32, act=1, f32=1),
    Lin("lin K 96: N 76, fp32 gelu_grad_of, scalar epilogue", "k_igemm2<128,32,4,1,32,3> g=3,3 v8=0 cm=0 dg=0", "ragged M, ragged N, N%8==4", 300, 76, 96,
        pg=2, f32=1),
    Lin("lin K 128: o_rowmap + residual + res_scale, 100 rows per sample", "k_igemm2<128,32,4,1,32,3> g=3,3 v8=1 cm=0 dg=0",
        "ragged M, ragged N, sample boundary", 300, 72, 128, maps=3, re=1, rps=100),
]


def _members(geos, flavour, dil):
    """geos: (B, Hs, Ws, Cin, Cout, k, s).  flavour "stats": statistics (dilated: statistics on the even members, an addend on the odd ones);
    "affine": scale / shift / residual / ReLU (dilated: the residual on the odd members only)."""
    out = []
    for i, (B, Hs, Ws, Cin, Cout, k, s) in enumerate(geos):
        kw = dict(d=1, Ho=2 * Hs - (i & 1), Wo=2 * Ws - ((i >> 1) & 1)) if dil else dict(s=s)
        if flavour == "stats":
            kw.update(st=0 if dil and (i & 1) else 1, ad=1 if dil and (i & 1) else 0)
        else:
            kw.update(entry="affine", re=(i & 1) if dil else (2 if i == 4 else 1), relu=1)
        out.append(Conv(f"member {i}", "", "", B, Hs, Ws, Cin, Cout, k, **kw))
    return out


# one-tile and one-pixel members, a member with three column tiles (Cout 72), Cout from {8, 20, 36, 72}, the last member's last tile ragged
_G32 = [(1, 1, 1, 8, 8, 1, 1), (2, 9, 7, 24, 20, 3, 1), (1, 20, 17, 40, 72, 3, 2), (3, 8, 6, 64, 36, 1, 2), (1, 19, 21, 16, 8, 3, 1), (4, 5, 5, 72, 20, 1, 1),
        (2, 13, 11, 8, 36, 3, 2), (1, 1, 1, 128, 72, 1, 1), (2, 6, 10, 32, 8, 3, 1), (1, 25, 9, 48, 20, 1, 2), (5, 3, 3, 24, 36, 3, 1), (1, 18, 15, 40, 72, 3, 1)]
_G64 = [(1, 1, 1, 192, 8, 1, 1), (2, 9, 7, 64, 20, 3, 1), (1, 20, 17, 64, 72, 3, 2), (3, 8, 6, 192, 36, 1, 2), (1, 19, 21, 64, 8, 3, 1), (4, 5, 5, 256, 20, 1, 1),
        (2, 13, 11, 128, 36, 3, 2), (1, 1, 1, 192, 72, 1, 1), (2, 6, 10, 64, 8, 3, 1), (1, 25, 9, 192, 20, 1, 2), (5, 3, 3, 128, 36, 3, 1), (1, 18, 15, 64, 72, 3, 1)]
GROUPS = [
    Group("group L3 BK32: statistics", "k_igemm2g<128,32,4,1,32,3> g=30,1 gy=1,1,3,2,1,1,2,3,1,1,2,3", "ragged M, ragged N, K tail, N%8==4, sample boundary",
          _members(_G32, "stats", False)),
    Group("group L3 BK64: scale shift residual ReLU", "k_igemm2g<128,32,4,1,64,3> g=30,1 gy=1,1,3,2,1,1,2,3,1,1,2,3",
          "ragged M, ragged N, N%8==4, sample boundary", _members(_G64, "affine", False)),
    Group("group L4 BK32: statistics / addend", "k_igemm2g<128,32,4,1,32,4> g=122,1 gy=1,1,3,2,1,1,2,3,1,1,2,3",
          "ragged M, ragged N, K tail, N%8==4, parity boundary", _members(_G32, "stats", True)),
    Group("group L4 BK64: scale shift residual ReLU", "k_igemm2g<128,32,4,1,64,4> g=122,1 gy=1,1,3,2,1,1,2,3,1,1,2,3",
          "ragged M, ragged N, N%8==4, parity boundary", _members(_G64, "affine", True)),
]
ALL = CONVS + LINS + GROUPS


def _id(c):
    return c.name.split(":")[0]


# ================================================================================================ the host check
def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def _route_fields(text):
    """'k_igemm2<128,64,4,1,64,3> g=3,1 v8=1 ...' -> (kernel, {key: value})"""
    parts = text.split()
    return parts[0], dict(p.split("=", 1) for p in parts[1:])


def _instantiation(kernel):
    """recorder's kernel name -> the key of the source's lists: ("tile" | "group", BM, BN, BK, LEAN), ("halo", CI, CO) or ("ring",)"""
    m = re.fullmatch(r"k_igemm2(g?)<(\d+),(\d+),\d+,\d+,(\d+),(\d+)>", kernel)
    if m:
        return ("group" if m.group(1) else "tile",) + tuple(int(v) for v in m.groups()[1:])
    m = re.fullmatch(r"k_conv3h<(\d+),(\d+)>", kernel)
    if m:
        return ("halo", int(m.group(1)), int(m.group(2)))
    assert kernel == "k_conv8p", kernel
    return ("ring",)


def test_case_tables_match_the_library(tmp_path):
    """No device is opened.  The launch recorder (the real entry points with the launch macro replaced by a printer) is fed every case: the
    kernel, tile, grid, v8 / cm / dg flags and statistics rows a case declares are what the library launches, and the instantiations the
    cases reach are exactly those that pk_igemm.hip names."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    lines, owner, sw = [], [], None
    for c in ALL:
        if c.sw != sw:
            sw = c.sw
            lines.append(f"switches sw={sw}")
            owner.append(None)
        lines.append(c.line())
        owner.append(c)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PK_CONV")}
    run = subprocess.run([exe, "--cases"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = run.stdout.splitlines()
    assert len(got) == len(lines)
    reached = {}
    for c, sent, rec in zip(owner, lines, got):
        assert rec.startswith(sent), (sent, rec)
        if c is None:
            continue
        parts = [p.strip() for p in rec[len(sent):].split(" | ")]
        assert len(parts) == 3 and parts[2].startswith("rc=0"), f"{c.name}: {rec}"
        kernel, want = _route_fields(c.route)
        launch = parts[1].split()
        assert launch[0] == kernel, f"{c.name}: declared {kernel}, the library launches {launch[0]}"
        have = dict(p.split("=", 1) for p in launch[1:] if "=" in p)
        gx, gy, gz = have["g"].split(",")
        assert gz == "1" and want["g"] == f"{gx},{gy}", f"{c.name}: declared grid {want['g']}, the library launches {have['g']}"
        if c.kind == "cgroup":
            assert int(have["n"]) == len(c.members) and int(have["end"]) == int(gx)
            members = re.findall(r"\[(\d+) gy=(\d+) v8=(\d) xr=0 cm=(\d) dg=(\d)\]", parts[1])
            assert len(members) == len(c.members)
            assert want["gy"] == ",".join(m[1] for m in members), f"{c.name}: gy {[m[1] for m in members]}"
            for m, (first, gy_, v8, cm, dg) in zip(c.members, members):
                # the documented flags of a member: v8 from the pointers, no chunk-major order, parity grouping for dilated 3x3 without statistics
                ptr_off = (m.re if m.entry == "affine" else m.ad) == 2
                assert (int(v8), int(cm), int(dg)) == (0 if ptr_off or m.Cout % 8 else 1, 0, 1 if m.d and m.k == 3 and not m.st else 0), (c.name, m.name)
        else:
            for key in ("v8", "cm", "dg"):
                assert want[key] == have[key], f"{c.name}: declared {key}={want[key]}, the library sets {have[key]}"
            if c.kind == "conv" and c.entry == "conv":
                rows = parts[2].split("rows=")[1]
                if c.d:        # pk_conv_stats_rows describes forward geometries; the dilated form writes ceil(M / 128) rows (no specialised kernel takes it)
                    rows = str((c.M + 127) // 128)
                assert want["rows"] == rows, f"{c.name}: declared rows={want['rows']}, the library says {rows}"
        reached.setdefault(_instantiation(kernel), []).append(c)
    with open(os.path.join(ROOT, "infantposeestimation_gaussianbias_amd", "csrc", "pk_igemm.hip")) as f:
        src = f.read()

    def tiles(macro):
        body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*)\n", src).group(1)
        return {tuple(int(v) for v in (a, b, e, f_)) for a, b, c_, d, e, f_ in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", body)}

    named = {("tile",) + t for t in tiles("IGEMM_TILES")} | {("group",) + t for t in tiles("IGEMM_GROUP_TILES")}
    launch_body = src[src.index("static int igemm_launch"):src.index("// ====", src.index("static int igemm_launch"))]
    named |= {("halo", int(a), int(b)) for a, b in re.findall(r"CONV3H_CASE\((\d+), (\d+)\)", launch_body)}
    assert "hipLaunchKernelGGL(k_conv8p" in launch_body
    named.add(("ring",))
    assert len(named) == 18 + 4 + 4 + 1, sorted(named)
    assert set(reached) == named, f"instantiations without a case: {sorted(named - set(reached))}; cases of unknown instantiations: {sorted(set(reached) - named)}"
    for inst, cases in reached.items():
        if inst[0] != "tile":
            continue
        have = {e for c in cases for e in c.edges}
        assert "ragged M" in have, f"{inst}: no case with a ragged last M tile"
        assert "ragged N" in have or inst[1] == 256, f"{inst}: no case with a ragged last N tile"          # (the 256-row tile's route asks for N % 128 == 0)
    have = {e for c in ALL for e in c.edges}
    assert have == set(EDGES), set(EDGES) - have
    # the declared edges are what the shapes have
    for c in CONVS + LINS:
        kernel, want = _route_fields(c.route)
        inst = _instantiation(kernel)
        N = c.Cout if c.kind == "conv" else c.N
        gx, gy = (int(v) for v in want["g"].split(","))
        if inst[0] == "tile":
            assert ("ragged M" in c.edges) == (c.M % inst[1] != 0), c.name
            assert ("ragged N" in c.edges) == (N % inst[2] != 0), c.name
            assert ("K tail" in c.edges) == (c.Cin % inst[3] != 0), c.name
            assert ("G%8==0" not in c.edges or gx * gy % 8 == 0) and ("G%8!=0" not in c.edges or gx * gy % 8 != 0), c.name          # (XCD tile order)
        assert ("N%8==4" in c.edges) == (N % 8 == 4), c.name
        if c.kind == "conv":
            assert ("parity boundary" in c.edges) == (want["dg"] == "1"), c.name
            if "sample boundary" in c.edges:
                assert c.B > 1 and (c.Ho * c.Wo) % 128 != 0, c.name


# ================================================================================================ data (made on the host: the same numbers on any device)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_data(rows, C, g):
    """[rows][C] of small integers: even channels from {0..3}, odd channels from {-3..3}"""
    nonneg = torch.randint(0, 4, (rows, C), generator=g)
    signed = torch.randint(-3, 4, (rows, C), generator=g)
    return torch.where(torch.arange(C) % 2 == 0, nonneg, signed).to(F32)


def chan_data(rows, C, g, offset=1.0):
    """[rows][C]: channel c ~ N(off_c, s_c^2), s_c = 10^U(-2, 2), |off_c| <= offset * s_c"""
    s = 10.0 ** (torch.rand(C, generator=g, dtype=F64) * 4 - 2)
    off = (torch.rand(C, generator=g, dtype=F64) * 2 - 1) * offset * s
    return (torch.randn(rows, C, generator=g, dtype=F64) * s + off).to(F32)


def guarded_view(data, guard_rows, dev, shift=0, named=None):
    """bf16 rows `data` between `guard_rows` NaN rows on either side, the view `shift` elements into a 16-byte aligned buffer (shift 4: the
    pointer sits 8 bytes off a 16-byte boundary); rows outside `named` (if given) are NaN as well.  -> (buffer, view)"""
    rows, C = data.shape
    data = data.to(BF)
    if named is not None:
        keep = torch.zeros(rows, dtype=torch.bool)
        keep[named] = True
        data[~keep] = NAN
    guard = -(-max(guard_rows, 1) * C // 8) * 8          # (whole 16-byte units: the view keeps the alignment `shift` gives it)
    buf = torch.full((2 * guard + rows * C + 8,), NAN, dtype=BF)
    buf[guard + shift:guard + shift + rows * C] = data.reshape(-1)
    buf = buf.to(dev)
    return buf, buf[guard + shift:guard + shift + rows * C].view(rows, C)


def vec_f32(values, dev, shift=0):
    """fp32 vector inside a NaN-guarded buffer, `shift` floats off a 16-byte boundary"""
    n = values.numel()
    buf = torch.full((n + 16,), NAN, dtype=F32)
    buf[8 + shift:8 + shift + n] = values.to(F32)
    buf = buf.to(dev)
    return buf, buf[8 + shift:8 + shift + n]


def pick(choices, n, g):
    return torch.tensor(choices, dtype=F32)[torch.randint(0, len(choices), (n,), generator=g)]


def weights(N, T, Cin, g, exact, flipped):
    """bf16 [N][T][Cin] inside a NaN-guarded buffer.  flipped: made as the weights src[n'][c'][t] of the forward layer (n' = Cin outputs,
    c' = N inputs) and packed as its data gradient reads them, dst[c'][T-1-t][n'] = src[n'][c'][t]."""
    shape = (Cin, N, T) if flipped else (N, Cin, T)
    if exact:
        src = torch.randint(-2, 3, shape, generator=g).to(F32) * (torch.rand(shape, generator=g) < 0.5)
    else:
        src = torch.randn(shape, generator=g) * (2.0 / math.sqrt(T * Cin))
    w = src.flip(2).permute(1, 2, 0) if flipped else src.permute(0, 2, 1)
    return w.contiguous().reshape(N, T * Cin)


def row_scales(n, g, exact):
    if exact:
        return pick([0.0, 0.5, 1.0, 2.0], n, g)
    s = (10.0 ** (torch.rand(n, generator=g) * 2 - 1)).float()
    s[0] = 0.0
    if n > 1:
        s[1] = 1.0 / 0.9          # DropPath's 1 / keep_prob: exact neither in bf16 nor in fp32
    return s


# ================================================================================================ references (float64, device-agnostic)
def conv_reference(xv, wv, c, dtype=F64):
    """xv [B Hs Ws][Cin], wv [N][T Cin] (bf16) -> acc, sum |a||w|: float64 / float32 [M][N].  One matmul per tap over strided slices of the
    zero-padded input; the dilated form zero-stuffs the input to (Ho, Wo) first and is then the same stride-1 contraction."""
    dev = xv.device
    x4 = xv.to(dtype).reshape(c.B, c.Hs, c.Ws, c.Cin)
    Hs, Ws, s = c.Hs, c.Ws, c.s
    if c.d:
        z = torch.zeros(c.B, c.Ho, c.Wo, c.Cin, dtype=dtype, device=dev)
        z[:, ::2, ::2] = x4
        x4, Hs, Ws, s = z, c.Ho, c.Wo, 1
    p = c.k // 2
    xp = torch.zeros(c.B, Hs + 2 * p, Ws + 2 * p, c.Cin, dtype=dtype, device=dev)
    xp[:, p:p + Hs, p:p + Ws] = x4
    w3 = wv.to(dtype).reshape(c.Cout, c.T, c.Cin)
    acc = torch.zeros(c.M, c.Cout, dtype=dtype, device=dev)
    ab = torch.zeros(c.M, c.Cout, dtype=F32, device=dev)          # (fp32 is exact for the integers below 2^24 and ample for a bound)
    for kh in range(c.k):
        for kw in range(c.k):
            a = xp[:, kh:kh + s * (c.Ho - 1) + 1:s, kw:kw + s * (c.Wo - 1) + 1:s].reshape(c.M, c.Cin)
            wt = w3[:, kh * c.k + kw].T
            acc += a @ wt
            ab += a.abs().float() @ wt.abs().float()
    return acc.double(), ab.double() * (1 + 2.0 ** -10)


def gelu64(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0)))


def gelu_grad64(v):
    return 0.5 * (1 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def softplus64(v):
    return torch.where(v > 30, v, torch.log1p(torch.exp(v.clamp_max(30))))


def tile_sums(v, rows_per_tile=128):
    """[M][N] -> [ceil(M / 128)][N]: sums over the rows of every statistics tile"""
    M, N = v.shape
    tiles = -(-M // rows_per_tile)
    pad = torch.zeros(tiles * rows_per_tile, N, dtype=v.dtype, device=v.device)
    pad[:M] = v
    return pad.reshape(tiles, rows_per_tile, N).sum(1)


def stats_reference(acc, E, adds=128):
    """-> ([tiles][2][N] reference, the same of its bound, the largest sum |v| and sum v^2 of a tile)"""
    ref = torch.stack([tile_sums(acc), tile_sums(acc * acc)], 1)
    mag = acc.abs() + E
    bs = tile_sums(E) + (adds + 16) * U * tile_sums(mag)
    bq = tile_sums(2 * acc.abs() * E + E * E) + (adds + 17) * U * tile_sums(mag * mag)
    return ref, torch.stack([bs, bq], 1), float(tile_sums(acc.abs()).max()), float(ref[:, 1].max())


def bf16_half_ulp(mag):
    """half an ulp of a bf16 number of magnitude `mag` (8 significant bits): 2^(floor(log2 mag) - 8), between 2^-9 mag and 2^-8 mag"""
    return torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** -126))) - 8)


class Expect:
    """What an epilogue must produce from the accumulators `acc` (error bound E): walks the documented order of operations."""

    def __init__(self, acc, E):
        self.v, self.e, self.inexact = acc, E, None

    def affine(self, scale, bias):
        if scale is None and bias is None:
            return
        s = torch.ones_like(self.v[0]) if scale is None else scale.double()
        b = torch.zeros_like(self.v[0]) if bias is None else bias.double()
        out = self.v * s + b
        self.e = self.e * s.abs() + 8 * U * (self.v.abs() * s.abs() + b.abs())
        self.v = out

    def stored(self, bf16, exact):
        """-> (expected stored value, its bound); the exact pass expects the value rounded once to bf16"""
        if not bf16:
            return self.v, self.e + 8 * U * self.v.abs()
        return (self.v.to(BF).double() if exact else self.v), self.e + bf16_half_ulp(self.v.abs() + self.e)

    def times_gelu_grad(self, z):
        gp = gelu_grad64(z.double())
        out = self.v * gp
        self.e = self.e * gp.abs() + self.v.abs() * ACT_TERM["gelu_grad"] * (1 + gp.abs()) + 8 * U * out.abs()
        self.v, self.inexact = out, "gelu_grad"

    def activation(self, name):
        fn, lip = (gelu64, GELU_LIP) if name == "gelu" else (softplus64, 1.0)
        out = fn(self.v)
        self.e = lip * self.e + ACT_TERM[name] * (1 + out.abs()) + 8 * U * out.abs()
        self.v, self.inexact = out, name

    def times(self, rs):
        self.v = self.v * rs
        self.e = self.e * rs.abs() + 8 * U * self.v.abs()

    def plus(self, res):
        self.e = self.e + 8 * U * (self.v.abs() + res.abs())
        self.v = self.v + res

    def relu(self):
        self.v = self.v.clamp_min(0)


# ================================================================================================ comparisons and guards
def agree(got, ref, bound, what, exact):
    """exact: got == ref everywhere (a NaN fails); otherwise |got - ref| <= bound element-wise"""
    kind = "bf16 stores" if got.dtype == BF else "fp32 results"
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
    if worst > WORST.get(kind, (0.0, ""))[0]:
        WORST[kind] = (worst, what)
    bad = ~(d <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(int(v) for v in idx[0])
        raise AssertionError(f"{what}: {idx.shape[0]} of {d.numel()} outside the bound; first at {i}: got {float(got[i])!r}, reference "
                             f"{float(ref[i])!r}, bound {float(bound[i])!r}; worst |error| / bound = {worst:.3g}")


def guarded(n, dtype, row):
    """n NaN elements, then a sentinel region of max(row, 4096) elements in the same allocation"""
    t = torch.full((n + max(row, 4096),), NAN, dtype=dtype, device=DEV)
    t[n:] = SENT
    return t


def intact(t, n, what):
    bad = t[n:] != SENT
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: written past its {n} elements: {int(bad.sum())} sentinels changed, first {i} elements past the end, "
                             f"now {float(t[n + i])!r}")


def written(t, n, what):
    intact(t, n, what)
    assert not bool(torch.isnan(t[:n]).any()), f"{what}: {int(torch.isnan(t[:n]).sum())} of {n} elements unwritten or NaN"
    return t[:n]


def same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is not None:
            it = torch.int16 if x.dtype == BF else torch.int32
            assert torch.equal(x.view(it), y.view(it)), f"{what}: two runs of the same launch differ"


def twice(launch, what):
    first = launch()
    torch.cuda.synchronize()
    second = launch()
    torch.cuda.synchronize()
    same_bits(first, second, what)
    return first


# ================================================================================================ convolutions
def conv_operands(c, exact, seed, dev):
    g = _gen(seed)
    o = {}
    flipped = bool(c.d) or (c.entry == "conv" and not c.st and not c.bi and c.s == 1 and c.om == 0)          # data gradients, stride 1 ones included
    xdata = int_data(c.B * c.Hs * c.Ws, c.Cin, g) if exact else chan_data(c.B * c.Hs * c.Ws, c.Cin, g)
    o["xbuf"], o["x"] = guarded_view(xdata, c.Hs * c.Ws, dev)
    o["wbuf"], o["w"] = guarded_view(weights(c.Cout, c.T, c.Cin, g, exact, flipped), 1, dev)
    o["bias"] = o["scale"] = o["res"] = None
    if c.bi or c.entry == "affine":
        vals = pick([-1.5, -0.5, 0.0, 0.5, 1.0, 2.5], c.Cout, g) if exact else torch.randn(c.Cout, generator=g) * 3
        o["bbuf"], o["bias"] = vec_f32(vals, dev, 1 if c.sc == 2 else 0)
    if c.entry == "affine":
        vals = pick([-1.0, 0.5, 1.0, 2.0], c.Cout, g) if exact else (10.0 ** (torch.rand(c.Cout, generator=g) * 2 - 1)) * pick([-1.0, 1.0], c.Cout, g)
        o["sbuf"], o["scale"] = vec_f32(vals, dev, 1 if c.sc == 2 else 0)
    off = c.re if c.entry == "affine" else c.ad
    if off:
        rdata = int_data(c.M, c.Cout, g) * 3 if exact else chan_data(c.M, c.Cout, g)
        o["rbuf"], o["res"] = guarded_view(rdata, c.Ho * c.Wo, dev, shift=4 if off == 2 else 0)
    return o


def conv_expect(c, o, exact, act, dtype=F64):
    """-> dict: out (value, bound, inexact), stats (reference, bound) or None; asserts the exact pass's premises on the reference"""
    acc, ab = conv_reference(o["x"], o["w"], c, dtype)
    assert not bool(torch.isnan(acc).any())
    E = torch.zeros_like(acc) if exact else (c.T * c.Cin + 16) * U * ab
    want = {"stats": None}
    if exact:
        assert float(ab.max()) < LIMIT, f"{c.name}: sum |a||w| reaches {float(ab.max())}"
    if c.st:
        halo = c.route.startswith("k_conv3h")
        ref, bound, s_abs, s_sq = stats_reference(acc, E, adds=c.M if halo else 128)
        if exact:
            assert s_abs < LIMIT and s_sq < LIMIT, f"{c.name}: a statistics tile reaches sum |v| = {s_abs}, sum v^2 = {s_sq}"
        want["stats"] = (ref, bound)
    e = Expect(acc, E)
    e.affine(o["scale"], o["bias"])
    if act == 2:
        e.activation("softplus")
    if c.om != 2:
        if o["res"] is not None:
            e.plus(o["res"].double())
        if c.relu:
            e.relu()
    v, b = e.stored(c.om == 0, exact)
    if exact:
        assert float(v.abs().max()) * 4 < LIMIT
    if c.om == 2:
        v, b = (t.reshape(c.B, c.Ho * c.Wo, c.Cout).permute(0, 2, 1).reshape(-1, c.Ho * c.Wo) for t in (v, b))
    want["out"] = (v, b, e.inexact)
    return want


def conv_launch(L, c, o, rows, act):
    n_out = c.M * c.Cout
    out = guarded(n_out, BF if c.om == 0 else F32, c.Cout if c.om != 2 else c.Ho * c.Wo)
    stats = guarded(rows * 2 * c.Cout, F32, 2 * c.Cout) if c.st else None
    if c.entry == "affine":
        L.call("pk_conv2d_affine_nhwc", o["x"], o["w"], out, o["scale"], o["bias"], o["res"], c.relu, c.B, c.Hs, c.Ws, c.Cin, c.Cout, c.k, c.s, c.Ho, c.Wo,
               L.stream_ptr())
    else:
        L.call("pk_conv2d_nhwc", o["x"], o["w"], out, stats, o["bias"], c.B, c.Hs, c.Ws, c.Cin, c.Cout, c.k, c.s, c.d, c.Ho, c.Wo, act, c.om, o["res"],
               L.stream_ptr())
    return out, stats


def check_conv_outputs(c, tag, want, out, stats, rows, exact):
    v, b, inexact = want["out"]
    got = written(out, c.M * c.Cout, f"{tag}: output").reshape(v.shape)
    if exact and inexact:          # behind an activation: the activation's term alone
        agree(got, v, b, f"{tag}: output behind {inexact}", False)
    else:
        agree(got, v, b, f"{tag}: output", exact)
    if c.st:
        ref, bound = want["stats"]
        got = written(stats, rows * 2 * c.Cout, f"{tag}: statistics ({rows} rows)").reshape(rows, 2, c.Cout)
        agree(got.double().sum(0), ref.sum(0), bound.sum(0), f"{tag}: float64 sum of the statistics rows", exact)
        if not c.route.startswith("k_conv3h"):
            assert rows == ref.shape[0], (rows, ref.shape)
            agree(got, ref, bound, f"{tag}: statistics rows", exact)


def run_conv(L, c, exact, seed):
    tag = f"{c.name} [{'exact' if exact else 'real'}]"
    o = conv_operands(c, exact, seed, DEV)
    rows = int(_route_fields(c.route)[1]["rows"]) if c.st else 0
    if c.st and not c.d:
        assert L.lib.pk_conv_stats_rows(c.B, c.Hs, c.Ws, c.Cin, c.Cout, c.k, c.s, c.Ho, c.Wo) == rows, f"{tag}: pk_conv_stats_rows"
    want = conv_expect(c, o, exact, c.act)
    out, stats = twice(lambda: conv_launch(L, c, o, rows, c.act), tag)
    check_conv_outputs(c, tag, want, out, stats, rows, exact)
    if exact and c.act:          # the twin without the activation: its pre-activation, exactly
        want = conv_expect(c, o, True, 0)
        out, stats = twice(lambda: conv_launch(L, c, o, rows, 0), tag + " twin")
        check_conv_outputs(c, tag + " twin without the activation", want, out, stats, rows, True)


@gpu
@pytest.mark.parametrize("case", CONVS, ids=[_id(c) for c in CONVS])
def test_conv_exact_then_real_with_guards(L, case, monkeypatch):
    if case.sw:
        monkeypatch.setenv("PK_CONV8P_MIN_TILES", "1")
        monkeypatch.setenv("PK_CONV3H_MIN_TILES", "1")
    seed = 1000 * CONVS.index(case)
    run_conv(L, case, True, seed)
    run_conv(L, case, False, seed + 500)


# ================================================================================================ linear layers
def lin_operands(c, exact, seed, dev):
    g = _gen(seed)
    o = {"a_map": None, "o_map": None, "res": None, "rs": None, "z": None}
    x_rows = out_rows = c.M
    named = None
    if c.maps == 2:          # a selection with repeats from 60 % of the source rows, -1 at 10 % of the places
        x_rows = c.M + 100
        pool = torch.randperm(x_rows, generator=g)[:x_rows * 6 // 10]
        m = pool[torch.randint(0, pool.numel(), (c.M,), generator=g)]
        m[torch.rand(c.M, generator=g) < 0.1] = -1
        named = m[m >= 0]
        o["a_map_host"], o["a_map"] = m, m.to(torch.int32).to(dev)
    if c.maps == 3:          # distinct destinations among more rows than M, -1 at 10 % of the places
        out_rows = c.M + 90
        m = torch.randperm(out_rows, generator=g)[:c.M]
        m[torch.rand(c.M, generator=g) < 0.1] = -1
        o["o_map_host"], o["o_map"] = m, m.to(torch.int32).to(dev)
    o["out_rows"] = out_rows
    dest = o["o_map_host"][o["o_map_host"] >= 0] if c.maps == 3 else None
    xdata = int_data(x_rows, c.K, g) if exact else chan_data(x_rows, c.K, g)
    o["xbuf"], o["x"] = guarded_view(xdata, 64, dev, named=named)
    o["wbuf"], o["w"] = guarded_view(weights(c.N, 1, c.K, g, exact, False), 1, dev)
    vals = pick([-1.5, -0.5, 0.0, 0.5, 1.0, 2.5], c.N, g) if exact else torch.randn(c.N, generator=g) * 3
    o["bbuf"], o["bias"] = vec_f32(vals, dev)
    if c.re:
        rdata = int_data(out_rows, c.N, g) * 3 if exact else chan_data(out_rows, c.N, g)
        o["rbuf"], o["res"] = guarded_view(rdata, 64, dev, named=dest)
        o["rsbuf"], o["rs"] = vec_f32(row_scales(-(-out_rows // c.rps), g, exact), dev)
    if c.pg == 2:
        zdata = int_data(out_rows, c.N, g) * 0.5 if exact else torch.randn(out_rows, c.N, generator=g) * 2
        o["zbuf"], o["z"] = guarded_view(zdata, 64, dev)
    return o


def lin_expect(c, o, exact, act, twin):
    with_z, want_pre = not twin, c.pg in (1, 3) or (twin and c.pg == 2)
    x = o["x"].double()
    if o["a_map"] is not None:
        src = o["a_map"].long()
        x = torch.where((src >= 0)[:, None], x[src.clamp_min(0)], torch.zeros((), dtype=F64, device=x.device))
    w = o["w"].double()
    acc, ab = x @ w.T, (x.abs().float() @ w.abs().float().T).double() * (1 + 2.0 ** -10)
    assert not bool(torch.isnan(acc).any())
    if exact:
        assert float(ab.max()) < LIMIT, f"{c.name}: sum |a||w| reaches {float(ab.max())}"
    E = torch.zeros_like(acc) if exact else (c.K + 16) * U * ab
    dest = torch.arange(c.M, device=x.device) if o["o_map"] is None else o["o_map"].long()
    live = dest >= 0
    e = Expect(acc, E)
    e.affine(None, o["bias"])
    want = {"live": live, "dest": dest, "preact": e.stored(True, exact) if want_pre else None}
    if with_z and o["z"] is not None:
        e.times_gelu_grad(o["z"][dest.clamp_min(0)])
    if act == 1:
        e.activation("gelu")
    if o["rs"] is not None:
        e.times(o["rs"].double()[dest.clamp_min(0) // c.rps][:, None])
    if o["res"] is not None:
        res = o["res"][dest.clamp_min(0)].double()
        e.plus(torch.where(live[:, None], res, torch.zeros((), dtype=F64, device=x.device)))
    v, b = e.stored(not c.f32, exact)
    if exact:
        assert float(v[live].abs().max()) * 4 < LIMIT
    want["out"] = (v, b, e.inexact)
    return want


def lin_launch(L, c, o, act, twin):
    """twin: the launch without GELU / gelu_grad_of; where gelu_grad_of is left out preact_out takes its place, which keeps the instantiation"""
    n = o["out_rows"] * c.N
    out = guarded(n, F32 if c.f32 else BF, c.N)
    pre = None
    if c.pg in (1, 3) or (twin and c.pg == 2):
        shift = 4 if c.pg == 3 else 0          # the view starts 8 bytes off a 16-byte boundary; NaN in front, sentinels behind its n elements
        pre = torch.full((shift + n + max(c.N, 4096),), NAN, dtype=BF, device=DEV)
        pre[shift + n:] = SENT
        pre = pre[shift:]
    L.call("pk_linear_bf16", o["x"], o["w"], out, o["bias"], o["res"], o["rs"], o["a_map"], o["o_map"], pre, None if twin else o["z"], c.M, c.N, c.K,
           c.rps, act, c.f32, L.stream_ptr())
    return out, pre


def check_lin_outputs(c, tag, o, want, out, pre, exact):
    n = o["out_rows"] * c.N
    live, dest = want["live"], want["dest"]
    for name, buf, size, exp in (("output", out, n, want["out"]), ("preact_out", pre, n, want["preact"])):
        if buf is None:
            continue
        intact(buf, size, f"{tag}: {name}")
        rows = buf[:n].reshape(o["out_rows"], c.N)
        named = torch.zeros(o["out_rows"], dtype=torch.bool, device=DEV)
        named[dest[live]] = True
        assert bool(torch.isnan(rows[~named]).all()), f"{tag}: {name}: a row no o_rowmap entry names was written"
        got = rows[dest[live]]
        assert not bool(torch.isnan(got).any()), f"{tag}: {name}: {int(torch.isnan(got).sum())} elements unwritten or NaN"
        v, b = exp[0][live], exp[1][live]
        if exact and name == "output" and exp[2]:
            agree(got, v, b, f"{tag}: output behind {exp[2]}", False)
        else:
            agree(got, v, b, f"{tag}: {name}", exact)


def run_lin(L, c, exact, seed):
    tag = f"{c.name} [{'exact' if exact else 'real'}]"
    o = lin_operands(c, exact, seed, DEV)
    want = lin_expect(c, o, exact, c.act, False)
    out, pre = twice(lambda: lin_launch(L, c, o, c.act, False), tag)
    check_lin_outputs(c, tag, o, want, out, pre, exact)
    if exact and (c.act or c.pg == 2) and c.pg not in (1, 3):          # no preact_out to hold the pre-activation: the twin launch does
        want = lin_expect(c, o, True, 0, True)
        out, pre = twice(lambda: lin_launch(L, c, o, 0, True), tag + " twin")
        check_lin_outputs(c, tag + " twin without the activation", o, want, out, pre, True)


@gpu
@pytest.mark.parametrize("case", LINS, ids=[_id(c) for c in LINS])
def test_linear_exact_then_real_with_guards(L, case):
    seed = 100000 + 1000 * LINS.index(case)
    run_lin(L, case, True, seed)
    run_lin(L, case, False, seed + 500)


# ================================================================================================ grouped convolutions
def run_group(L, grp, exact, seed):
    from infantposeestimation_gaussianbias_amd import exchange
    ops = [conv_operands(m, exact, seed + 10 * i, DEV) for i, m in enumerate(grp.members)]
    wants = []
    for m, o in zip(grp.members, ops):
        m.route = "k_igemm2g"          # (statistics rows per 128 output pixels, like the tile family)
        wants.append(conv_expect(m, o, exact, 0))
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731

    def launch():
        rows, bufs = [], []
        for m, o in zip(grp.members, ops):
            tiles = L.lib.pk_conv_stats_tiles(m.M)
            out = guarded(m.M * m.Cout, BF, m.Cout)
            stats = guarded(tiles * 2 * m.Cout, F32, 2 * m.Cout) if m.st else None
            rows.append(dict(x=p(o["x"]), w=p(o["w"]), out=p(out), stats=p(stats), col_scale=p(o["scale"]), bias=p(o["bias"]), res=p(o["res"]), B=m.B,
                             Hs=m.Hs, Ws=m.Ws, Cin=m.Cin, Cout=m.Cout, ksize=m.k, stride=m.s, dilated_input=m.d, Ho=m.Ho, Wo=m.Wo,
                             act=3 if m.relu else 0))
            bufs += [out, stats]
        exchange._launch("pk_conv2d_group", exchange.CONV_DT, rows)
        return bufs

    bufs = twice(launch, grp.name)
    for i, (m, want) in enumerate(zip(grp.members, wants)):          # each member on its own against its reference
        tag = f"{grp.name} member {i} {(m.B, m.Hs, m.Ws, m.Cin, m.Cout, m.k, m.s, m.d)} [{'exact' if exact else 'real'}]"
        check_conv_outputs(m, tag, want, bufs[2 * i], bufs[2 * i + 1], L.lib.pk_conv_stats_tiles(m.M), exact)


@gpu
@pytest.mark.parametrize("grp", GROUPS, ids=[_id(g) for g in GROUPS])
def test_group_members_exact_then_real(L, grp):
    assert len(grp.members) == 12
    seed = 200000 + 1000 * GROUPS.index(grp)
    run_group(L, grp, True, seed)
    run_group(L, grp, False, seed + 500)


# ================================================================================================ host-only: the exact pass's premises
def test_exact_operands_stay_below_2_24():
    """No device: the exact pass's operands, made on the host, keep sum |a||w| of every output, sum |v| and sum v^2 of every statistics
    tile and every expected output below 2^24 (the assertions sit in conv_expect / lin_expect, which the GPU tests run as well).  The three
    cases of ~30 000 x 1152 outputs accumulate in fp32 here (exact below 2^24, which is what is asserted) to keep the host test short."""
    for i, c in enumerate(CONVS):
        conv_expect(c, conv_operands(c, True, 1000 * i, "cpu"), True, 0, F32 if c.M * c.Cout * c.T * c.Cin > 1e10 else F64)
    for i, c in enumerate(LINS):
        lin_expect(c, lin_operands(c, True, 100000 + 1000 * i, "cpu"), True, 0, True)
    for j, grp in enumerate(GROUPS):
        for i, m in enumerate(grp.members):
            m.route = "k_igemm2g"
            conv_expect(m, conv_operands(m, True, 200000 + 1000 * j + 10 * i, "cpu"), True, 0)


# ================================================================================================ the activations' own error
@gpu
def test_activation_error_is_measured(L):
    """GELU, gelu' and softplus over EVERY finite bf16 pre-activation of magnitude <= 32, fp32 output, against float64.  Identity weights (and
    no bias) make the fp32 pre-activation the bf16 input itself, so the difference is the activation code's alone (plus the fp32 rounding
    of the result).  ACT_TERM holds four times the recorded measurement and may not pass 2^-16 (1 + |ref|)."""
    bits = torch.arange(0, 0x4200 + 1, dtype=torch.int32)
    vals = torch.cat([bits, bits + 0x8000]).to(torch.int16).view(BF)
    vals = vals[torch.randperm(vals.numel(), generator=_gen(7))]
    C = 32
    M = vals.numel() // C
    z = vals[:M * C].reshape(M, C).to(DEV).contiguous()
    eye = torch.eye(C, dtype=BF, device=DEV)
    ones = torch.ones(M, C, dtype=BF, device=DEV)
    z64 = z.double()

    def measure(name, got, ref):
        assert not bool(torch.isnan(got).any())
        worst = float(((got.double() - ref).abs() / (1 + ref.abs())).max())
        ACT_SEEN[name] = worst
        print(f"{name}: worst |error| / (1 + |ref|) = {worst:.3g} over {got.numel()} bf16 pre-activations")
        assert ACT_TERM[name] <= ACT_CAP, f"{name}: the term {ACT_TERM[name]} passes the cap 2^-16"
        assert worst <= ACT_TERM[name], f"{name}: measured {worst}, term {ACT_TERM[name]}"

    out = guarded(M * C, F32, C)
    L.call("pk_linear_bf16", z, eye, out, None, None, None, None, None, None, None, M, C, C, 0, 1, 1, L.stream_ptr())
    torch.cuda.synchronize()
    measure("gelu", written(out, M * C, "gelu").reshape(M, C), gelu64(z64))
    out = guarded(M * C, F32, C)
    L.call("pk_linear_bf16", ones, eye, out, None, None, None, None, None, None, z, M, C, C, 0, 0, 1, L.stream_ptr())
    torch.cuda.synchronize()
    measure("gelu_grad", written(out, M * C, "gelu_grad").reshape(M, C), gelu_grad64(z64))
    out = guarded(M * C, F32, M)
    L.call("pk_conv2d_nhwc", z, eye, out, None, None, 1, M, 1, C, C, 1, 1, 0, M, 1, 2, 2, None, L.stream_ptr())
    torch.cuda.synchronize()
    measure("softplus", written(out, M * C, "softplus").reshape(C, M).T, softplus64(z64))
