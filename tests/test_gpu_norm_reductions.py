"""GPU tests (`-m gpu`) of the normalisation and partial-sum kernels of csrc/pk_bn.hip and csrc/pk_ln.hip at the row counts training runs.

The library picks its code path from the tensor size (release builds have no run-time switch), so every case here is chosen by size:
the fused one-launch BatchNorm paths (tiles <= 128 and rows <= 32768 forward, rows <= 32768 backward), the multi-launch paths behind
them (k_bn_finalize + k_bn_act; k_bn_bwd_reduce over up to 1024 blocks + k_sum_partials + k_bn_bwd_apply), the grouped entries of the
exchange units, LayerNorm and the column sums at 1024 blocks.  Entries are called through the C-ABI directly.

References are float64 ATen on the device, fed the exact bf16 / fp32 values the kernel reads.  Data has a scale per channel spread
over 10^-2 .. 10^2 and a mean offset per channel of up to 8 standard deviations, and every comparison is per element or per channel
against a bound derived from the fp32 / bf16 roundings the kernel performs (U = 2^-24, the fp32 unit roundoff):
  * a fp32 sum along a serial chain of L additions is within L*U*sum|term| of the exact sum; the chain lengths follow from the launch
    shape (row lanes of a workgroup, rows per block), which the helpers below restate;
  * a bf16 store adds at most one bf16 ulp of the reference (half an ulp of the stored value, which is at most one of the reference).
Output buffers start as NaN, so a dropped write fails its comparison.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
EPS = float(np.float32(1e-5))          # the eps / momentum the kernels receive, as fp32
MOM = float(np.float32(0.1))
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


def call(L, name, *args):
    L.call(name, *args, L.stream_ptr())


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def chan_data(rows, C, seed, offset=8.0):
    """bf16 [rows][C]: channel c ~ N(off_c, s_c^2), s_c = 10^U(-2, 2), |off_c| <= offset * s_c"""
    g = gen(seed)
    s = 10.0 ** (torch.rand(C, generator=g, device=DEV, dtype=F64) * 4 - 2)
    off = (torch.rand(C, generator=g, device=DEV, dtype=F64) * 2 - 1) * offset * s
    return (torch.randn(rows, C, generator=g, device=DEV, dtype=F32).double() * s + off).to(BF)


def affine(C, seed):
    """fp32 gamma (signed, |gamma| = 10^U(-1, 1)) and beta"""
    g = gen(seed)
    sign = torch.where(torch.rand(C, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    gamma = (sign * 10.0 ** (torch.rand(C, generator=g, device=DEV) * 2 - 1)).float()
    beta = torch.randn(C, generator=g, device=DEV).float()
    return gamma, beta


def nan_like(t):
    return torch.full_like(t, NAN)


def ulp_bf16(v):
    """bf16 ulp at |v| (0 at 0)"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.exp2((e - 8).to(v.dtype)))


def ulp_f32(v):
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.exp2((e - 24).to(v.dtype)))


def within(got, ref, bound, what):
    """|got - ref| <= bound element-wise (a NaN in `got` fails)"""
    d = (got.double() - ref).abs()
    bad = ~(d <= bound)
    print(f"{what}: worst |error| / bound {float((d / bound.clamp_min(1e-300)).max()):.3g}")
    if bool(bad.any()):
        n = int(bad.sum())
        i = int(bad.reshape(-1).nonzero()[0])
        g_, r_, b_ = (float(t.reshape(-1)[i]) for t in (got.double(), ref, bound))
        worst = float((d / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max())
        raise AssertionError(f"{what}: {n} of {d.numel()} outside the bound; first at flat index {i}: got {g_!r}, reference {r_!r}, "
                             f"bound {b_!r}; worst |error| / bound = {worst:.3g}")


def mask_bits(y):
    """relu_mask layout: one byte per 8 channels, bit j = channel j of the chunk is > 0 in the stored y"""
    rows, C = y.shape
    pos = (y.float() > 0).reshape(rows, C // 8, 8).to(torch.int32)
    return (pos << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1).to(torch.uint8).reshape(-1)


def chain(rows, nb, row_lanes):
    """fp32 serial chain of a block-partial reduction: each row lane adds ceil(rows_per_block / row_lanes) terms, then one lane adds the
    row_lanes lane sums; the partials are combined in float64 and rounded once"""
    rpb = -(-rows // nb)
    return -(-rpb // row_lanes) + row_lanes


def ln_lanes(C):
    """lanes per row of the LayerNorm kernels (the launch layout of pk_layernorm_fwd / _bwd; used only to size the error bounds)"""
    if C > 512:
        return 64, 2
    lanes = 1
    while lanes * 8 < C and lanes < 64:
        lanes *= 2
    return lanes, 1


def conv_tiles(L, geom):
    return geom if isinstance(geom, int) else L.lib.pk_conv_stats_rows(*geom)


# ================================================================================================ BatchNorm forward
def stats_partials(raw, tiles):
    """the conv epilogue's statistics: per tile (rows split into `tiles` contiguous runs, possibly empty) float64 sum x and sum x^2 of
    the bf16 raw values, stored as fp32"""
    rows, C = raw.shape
    x = raw.double()
    tid = torch.arange(rows, device=DEV) * tiles // rows
    s = torch.zeros(tiles, C, dtype=F64, device=DEV).index_add_(0, tid, x)
    q = torch.zeros(tiles, C, dtype=F64, device=DEV).index_add_(0, tid, x * x)
    return torch.stack([s, q], 1).float().contiguous()


class FwdCase:
    def __init__(self, rows, tiles, C, relu, res, mask, seed):
        self.rows, self.tiles, self.C, self.relu, self.use_mask = rows, tiles, C, relu, mask
        self.raw = chan_data(rows, C, seed)
        self.part = stats_partials(self.raw, tiles)
        self.gamma, self.beta = affine(C, seed + 1)
        self.res = chan_data(rows, C, seed + 2, offset=1.0) if res else None
        P = self.part.double()
        self.S, self.Q = P[:, 0].sum(0), P[:, 1].sum(0)                   # fp64 of the SAME fp32 partials
        self.mean = self.S / rows
        self.var = (self.Q / rows - self.mean ** 2).clamp_min(0)
        self.rstd = 1 / torch.sqrt(self.var + EPS)
        self.abs_s, self.abs_q = P[:, 0].abs().sum(0), P[:, 1].sum(0)
        g = gen(seed + 3)
        self.rm0 = (self.mean * (0.5 + torch.rand(C, generator=g, device=DEV, dtype=F64))).float()
        self.rv0 = (self.var * (0.5 + torch.rand(C, generator=g, device=DEV, dtype=F64))).float()

    def buffers(self):
        C = self.C
        return dict(y=nan_like(self.raw), mean=torch.full((C,), NAN, device=DEV), rstd=torch.full((C,), NAN, device=DEV),
                    rm=self.rm0.clone(), rv=self.rv0.clone(), scale=torch.full((C,), NAN, device=DEV), shift=torch.full((C,), NAN, device=DEV),
                    mask=torch.full((self.rows * C // 8,), 0xA5, dtype=torch.uint8, device=DEV) if self.use_mask else None)

    def desc(self, b, nbt):
        p = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
        return dict(raw=p(self.raw), stats_partial=p(self.part), gamma=p(self.gamma), beta=p(self.beta), running_mean=p(b["rm"]),
                    running_var=p(b["rv"]), num_batches_tracked=p(nbt), residual=p(self.res), y=p(b["y"]), save_mean=p(b["mean"]),
                    save_rstd=p(b["rstd"]), relu_mask=p(b["mask"]), rows=self.rows, tiles=self.tiles, C=self.C, momentum=MOM, eps=EPS,
                    relu=1 if self.relu else 0)

    def run_single(self, L, b, nbt):
        call(L, "pk_bn_train_fwd", self.raw, self.part, self.tiles, self.C, self.rows, self.gamma, self.beta, b["rm"], b["rv"], nbt, MOM, EPS,
             self.res, b["y"], b["mean"], b["rstd"], b["scale"], b["shift"], 1 if self.relu else 0, b["mask"])

    def check(self, b):
        rows, C = self.rows, self.C
        # save_mean / save_rstd vs float64 of the same fp32 partials: the kernel's rounding to fp32 (2 ulp) plus its own float64 summation
        # order over the partials (2^-50 of the magnitudes summed)
        within(b["mean"], self.mean, 2 * ulp_f32(self.mean) + 2.0 ** -50 * self.abs_s / rows, "save_mean vs fp64 of the partials")
        dvar = 2.0 ** -50 * self.abs_q / rows
        within(b["rstd"], self.rstd, 2 * ulp_f32(self.rstd) + self.rstd * dvar / (self.var + EPS), "save_rstd vs fp64 of the partials")
        # ... and vs the true statistics of raw: each partial carries one fp32 rounding (<= U of its magnitude)
        x = self.raw.double()
        mt, vt = x.mean(0), x.var(0, unbiased=False)
        dm = U * self.abs_s / rows
        dv = U * self.abs_q / rows + 2 * mt.abs() * dm + dm * dm
        within(b["mean"], mt, 2 * ulp_f32(mt) + dm, "save_mean vs the statistics of raw")
        rt = 1 / torch.sqrt(vt + EPS)
        within(b["rstd"], rt, 2 * ulp_f32(rt) + 0.51 * rt * dv / (vt + EPS), "save_rstd vs the statistics of raw")
        # running statistics: momentum 0.1 and the UNBIASED batch variance; reference with the kernel's fp32 constants 0.1f and 1 - 0.1f
        keep = float(np.float32(1) - np.float32(MOM))
        unb = self.var * (rows / (rows - 1)) if rows > 1 else self.var
        for got, old, new, what in ((b["rm"], self.rm0, self.mean, "running_mean"), (b["rv"], self.rv0, unb, "running_var")):
            ref = keep * old.double() + MOM * new
            within(got, ref, 2 * ulp_f32(old.double().abs() + ref.abs()), what)
        # y per element: one bf16 ulp + the fp32 roundings.  x*scale: rstd, gamma*rstd and the product (3 U |x*scale|); shift =
        # beta - ((mean*gamma)*rstd): mean, rstd, two products and the difference (4 U |mean*scale| + U |shift|); the sum with shift and
        # the residual (U each of |t|).  With |shift| <= |beta| + |mean*scale| that is at most 8 U (|x*scale| + |mean*scale| + |beta| + |res|)
        scale = self.gamma.double() * self.rstd
        xs = x * scale
        t = xs + (self.beta.double() - self.mean * scale)
        if self.res is not None:
            t = t + self.res.double()
        ref = t.clamp_min(0) if self.relu else t
        rb = 0 if self.res is None else self.res.double().abs()
        bound = ulp_bf16(ref) + 8 * U * (xs.abs() + self.beta.double().abs() + (self.mean * scale).abs() + rb)
        within(b["y"], ref, bound, "y")
        if b["mask"] is not None:
            assert torch.equal(b["mask"], mask_bits(b["y"])), "relu_mask is not the > 0 pattern of the stored y"

    def fused(self):
        return self.tiles <= 128 and self.rows <= 32768


FWD_CASES = [  # rows, tiles (int or the conv geometry whose pk_conv_stats_rows it is), C, relu, residual, relu_mask
    (1, 1, 8, True, True, True),               # fused; one row: zero variance, count - 1 == 0
    (7, 128, 24, False, False, False),         # fused; 121 empty tiles
    (7, 3000, 136, True, False, True),         # two launches with far more stats rows than rows
    (129, 129, 40, True, True, False),         # one stats row over the fused limit
    (129, 1, 8, False, True, True),
    (32768, 128, 64, True, False, True),       # both fused limits exactly
    (32768, 129, 136, False, True, False),
    (32768, 1, 1024, True, True, True),        # fused, 32 channel groups
    (32769, 128, 32, True, True, True),        # one row over the fused limit
    (32769, 1, 1024, False, False, False),
    (196608, (64, 64, 48, 64, 64, 3, 1, 64, 48), 64, True, False, True),       # HRFormer-small branch 0 (64x48, B = 64), 3x3 64 -> 64
    (196608, (64, 64, 48, 64, 256, 1, 1, 64, 48), 256, True, True, True),      # layer1 bottleneck 1x1 64 -> 256 + skip
    (196608, 3000, 40, False, False, True),
    (221184, (32, 96, 72, 32, 32, 3, 1, 96, 72), 32, True, True, True),        # HRNet-W32 branch 0 BasicBlock (96x72, B = 32)
    (221184, 129, 24, False, True, False),
]


@pytest.mark.parametrize("rows,tiles,C,relu,res,mask", FWD_CASES)
def test_bn_train_fwd_both_paths_vs_fp64(L, rows, tiles, C, relu, res, mask):
    case = FwdCase(rows, conv_tiles(L, tiles), C, relu, res, mask, seed=rows + 7 * C)
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    runs = []
    for rep in range(2):
        b = case.buffers()
        case.run_single(L, b, nbt)
        torch.cuda.synchronize()
        assert int(nbt) == 6 + rep, "num_batches_tracked must grow by exactly one per call"
        # path witness: only the two-launch path (k_bn_finalize + k_bn_act) writes the scale / shift workspaces
        if case.fused():
            assert bool(torch.isnan(b["scale"]).all() and torch.isnan(b["shift"]).all()), "fused path expected, workspaces were written"
        else:
            assert torch.equal(b["scale"], case.gamma * b["rstd"]), "scale != gamma * rstd"
            assert torch.equal(b["shift"], case.beta - b["mean"] * case.gamma * b["rstd"]), "shift != beta - mean * gamma * rstd"
        runs.append(b)
    case.check(runs[0])
    for k, v in runs[0].items():
        if v is not None:
            assert torch.equal(v.view(torch.uint8), runs[1][k].view(torch.uint8)), f"{k} differs between two identical calls"


# ================================================================================================ BatchNorm backward
class BwdCase:
    def __init__(self, rows, C, relu, seed):
        self.rows, self.C, self.relu = rows, C, relu
        self.raw = chan_data(rows, C, seed)
        x = self.raw.double()
        self.mean = x.mean(0).float()                                   # the forward's saved statistics (fp32)
        self.rstd = (1 / torch.sqrt(x.var(0, unbiased=False) + EPS)).float()
        self.gamma, beta = affine(C, seed + 1)
        self.y = ((x - self.mean.double()) * self.rstd.double() * self.gamma.double() + beta.double()).to(BF)
        self.bits = mask_bits(self.y)
        self.dy = chan_data(rows, C, seed + 2)

    def buffers(self, nb, dres):
        return dict(part=torch.full((nb, 2, self.C), NAN, device=DEV), sums=torch.full((2 * self.C,), NAN, device=DEV),
                    dgamma=torch.full((self.C,), NAN, device=DEV), dbeta=torch.full((self.C,), NAN, device=DEV), dx=nan_like(self.raw),
                    dres=nan_like(self.raw) if dres else None)

    def flags(self, eval_mode):
        return (1 if self.relu else 0) | (2 if eval_mode else 0)

    def run_single(self, L, b, use_mask, eval_mode):
        call(L, "pk_bn_bwd", self.dy, None if use_mask else self.y, self.raw, self.mean, self.rstd, self.gamma, b["part"], b["sums"],
             b["dgamma"], b["dbeta"], b["dx"], b["dres"], self.rows, self.C, self.flags(eval_mode), self.bits if use_mask else None)

    def desc(self, b, use_mask):
        p = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
        return dict(dy=p(self.dy), y_act=0 if use_mask else p(self.y), raw=p(self.raw), save_mean=p(self.mean), save_rstd=p(self.rstd),
                    gamma=p(self.gamma), partial=p(b["part"]), dgamma=p(b["dgamma"]), dbeta=p(b["dbeta"]), dx=p(b["dx"]),
                    dresidual=p(b["dres"]), relu_mask=p(self.bits) if use_mask else 0, rows=self.rows, C=self.C, relu=self.flags(False))

    def check(self, b, nb, eval_mode=False):
        rows, C = self.rows, self.C
        pos = self.y.float() > 0 if self.relu else torch.ones_like(self.raw, dtype=torch.bool)
        g = torch.where(pos, self.dy.double(), 0.0)
        mu, rs, gam = self.mean.double(), self.rstd.double(), self.gamma.double()
        xh = (self.raw.double() - mu) * rs
        gx = g * xh
        # dgamma / dbeta: fp32 chain of the block reduction (k_bn_bwd_reduce: 256 / (C/8) row lanes) + the fp32 x-hat and product
        # roundings of each term (3) + the final rounding (1).  At the production shapes (192 rows per block) that is 36 .. 42 U, about
        # 2.5e-6 of sum|term|, where dropping one block moves the sum by ~1e-3; the small path at C = 8 or 1024 (512 rows per block, 256
        # or 2 row lanes) has a chain of 258 and a bound of 1.6e-5
        Lc = chain(rows, nb, 256 // (C // 8)) + 4
        sg, sgx = g.sum(0), gx.sum(0)
        eg, egx = Lc * U * g.abs().sum(0), Lc * U * gx.abs().sum(0)
        within(b["dbeta"], sg, eg, "dbeta")
        within(b["dgamma"], sgx, egx, "dgamma")
        gm = gam * rs
        if eval_mode:
            # running statistics are constants: dx = gamma * rstd * g (two fp32 roundings, one bf16 store)
            ref = gm * g
            within(b["dx"], ref, ulp_bf16(ref) + 2 * U * ref.abs(), "dx (eval mode)")
        else:
            t1, t2 = sg / rows, sgx / rows
            ref = gm * (g - t1 - xh * t2)
            dt1, dt2 = eg / rows + 2 * U * t1.abs(), egx / rows + 2 * U * t2.abs()
            bound = ulp_bf16(ref) + gm.abs() * (4 * U * (g.abs() + t1.abs() + (xh * t2).abs()) + dt1 + xh.abs() * dt2) + 2 * U * ref.abs()
            within(b["dx"], ref, bound, "dx")
        if b["dres"] is not None:
            assert torch.equal(b["dres"].view(torch.int16), torch.where(pos, self.dy, torch.zeros_like(self.dy)).view(torch.int16)), \
                "dresidual is not the masked dy"


BWD_CASES = [  # rows, C, relu, dresidual
    (1, 8, True, True), (7, 24, True, False), (129, 136, False, True), (32768, 8, True, True), (32768, 64, True, False),
    (32768, 1024, True, True), (32769, 24, True, True), (32769, 136, True, False), (40000, 40, False, True),
    (196608, 64, True, True), (196608, 256, True, False), (221184, 32, True, True)]


@pytest.mark.parametrize("rows,C,relu,dres", BWD_CASES)
def test_bn_bwd_both_paths_vs_fp64(L, rows, C, relu, dres):
    case = BwdCase(rows, C, relu, seed=3 * rows + C)
    nb = L.lib.pk_bn_bwd_blocks(rows)
    runs = []
    for use_mask in ([False, True] if relu else [False]):
        b = case.buffers(nb, dres)
        case.run_single(L, b, use_mask, False)
        torch.cuda.synchronize()
        # path witness: only the large-tensor path (k_bn_bwd_reduce + k_sum_partials + k_bn_bwd_apply) writes `sums`
        if rows <= 32768:
            assert bool(torch.isnan(b["sums"]).all()), "small path expected, sums was written"
        else:
            assert torch.equal(b["sums"], torch.cat([b["dbeta"], b["dgamma"]])), "sums != [dbeta | dgamma]"
        runs.append(b)
    case.check(runs[0], nb)
    if relu:        # dx through relu_mask == dx through y_act: both masks come from the same stored y
        for k in ("dx", "dres", "dgamma", "dbeta"):
            if runs[0][k] is not None:
                assert torch.equal(runs[0][k].view(torch.uint8), runs[1][k].view(torch.uint8)), f"{k}: relu_mask path != y_act path"


@pytest.mark.parametrize("rows,C", [(7, 24), (32768, 64), (196608, 64)])
def test_bn_bwd_eval_mode_both_paths(L, rows, C):
    case = BwdCase(rows, C, True, seed=rows + 11 * C)
    nb = L.lib.pk_bn_bwd_blocks(rows)
    b = case.buffers(nb, True)
    case.run_single(L, b, True, True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(b["sums"]).all()) == (rows <= 32768)
    case.check(b, nb, eval_mode=True)


# ================================================================================================ grouped entries
def _group(L, name, dt, rows_):
    arr = np.zeros(len(rows_), dtype=dt)
    for i, r in enumerate(rows_):
        for k, v in r.items():
            arr[i][k] = v
    L.call(name, arr.ctypes.data, len(rows_), L.stream_ptr())


def test_grouped_bn_members_vs_fp64_and_single_entries(L):
    from infantposeestimation_gaussianbias_amd import exchange
    branch0 = L.lib.pk_conv_stats_rows(64, 64, 48, 32, 32, 3, 1, 64, 48)      # HRFormer-small branch 0 at 64x48, B = 64, 3x3 32 -> 32
    spec = [  # rows, tiles, C, relu, residual, relu_mask (forward and backward)
        (240, L.lib.pk_conv_stats_tiles(240), 32, True, True, True),
        (32769, 257, 64, True, False, False),
        (196608, branch0, 32, True, True, True),
        (3000, 24, 136, False, False, False),
        (32768, 128, 24, True, False, True)]
    fwd = [FwdCase(r, t, c, relu, res, m, seed=100 + i) for i, (r, t, c, relu, res, m) in enumerate(spec)]
    nbt_s = torch.zeros(len(spec), dtype=torch.int64, device=DEV)
    nbt_g = torch.zeros(len(spec), dtype=torch.int64, device=DEV)
    single, grouped = [c.buffers() for c in fwd], [c.buffers() for c in fwd]
    for i, c in enumerate(fwd):
        c.run_single(L, single[i], nbt_s[i])
    _group(L, "pk_bn_train_fwd_group", exchange.BNF_DT, [c.desc(grouped[i], nbt_g[i]) for i, c in enumerate(fwd)])
    torch.cuda.synchronize()
    assert nbt_g.tolist() == [1] * len(spec) and nbt_s.tolist() == [1] * len(spec)
    for i, c in enumerate(fwd):
        c.check(grouped[i])
        c.check(single[i])
        if c.fused():       # the single entry's fused path: the same bn_act_fin_body on the same grid
            for k in ("y", "mean", "rstd", "rm", "rv", "mask"):
                if grouped[i][k] is not None:
                    assert torch.equal(grouped[i][k].view(torch.uint8), single[i][k].view(torch.uint8)), f"member {i}: {k} != single entry"

    bwd = [BwdCase(r, c, relu, seed=200 + i) for i, (r, _, c, relu, _, _) in enumerate(spec)]
    single, grouped = [], []
    for i, (c, s) in enumerate(zip(bwd, spec)):
        use_mask, dres = s[5], s[4]
        bs = c.buffers(L.lib.pk_bn_bwd_blocks(c.rows), dres)
        c.run_single(L, bs, use_mask, False)
        single.append(bs)
        grouped.append(c.buffers(L.lib.pk_bn_bwd_group_blocks(c.rows), dres))
    _group(L, "pk_bn_bwd_group", exchange.BNB_DT, [c.desc(grouped[i], spec[i][5]) for i, c in enumerate(bwd)])
    torch.cuda.synchronize()
    for i, c in enumerate(bwd):
        c.check(grouped[i], L.lib.pk_bn_bwd_group_blocks(c.rows))
        c.check(single[i], L.lib.pk_bn_bwd_blocks(c.rows))
        if c.rows <= 32768:     # pk_bn_bwd_group_blocks: "same sums bit for bit" where the small-tensor rule applies
            for k in ("dx", "dres", "dgamma", "dbeta"):
                if grouped[i][k] is not None:
                    assert torch.equal(grouped[i][k].view(torch.uint8), single[i][k].view(torch.uint8)), f"member {i}: {k} != single entry"


# ================================================================================================ LayerNorm
@pytest.mark.parametrize("rows", [196608, 3 * 1024 + 5])
@pytest.mark.parametrize("C,Cr", [(32, 32), (64, 64), (80, 78), (640, 640)])
def test_layernorm_fwd_bwd_many_blocks_vs_fp64(L, rows, C, Cr):
    seed = rows + C
    x = chan_data(rows, C, seed)
    dy, dres = chan_data(rows, C, seed + 1), chan_data(rows, C, seed + 2, offset=1.0)
    for t in (x, dy, dres):
        t[:, Cr:] = 0                                  # padded inputs are zero
    gamma, beta = affine(C, seed + 3)
    gamma[Cr:], beta[Cr:] = 7.0, 3.0                   # padded entries must be ignored
    y, mean, rstd = nan_like(x), torch.full((rows,), NAN, device=DEV), torch.full((rows,), NAN, device=DEV)
    call(L, "pk_layernorm_fwd", x, gamma, beta, y, mean, rstd, rows, C, Cr, EPS)
    lanes, cpl = ln_lanes(C)
    Lr = 8 * cpl + int(math.log2(lanes))               # fp32 chain of a per-row sum: 8 * CPL serial terms per lane, then a lane butterfly
    xr = x[:, :Cr].double()
    mu, var = xr.mean(1), xr.var(1, unbiased=False)
    r64 = 1 / torch.sqrt(var + EPS)
    dmu = (Lr + 1) * U * xr.abs().sum(1) / Cr
    within(mean, mu, dmu + ulp_f32(mu), "LayerNorm mean")
    # rstd: the mean error cancels to first order in sum (x - mean)^2; chain + 3 roundings per term and the division, then half of that
    # through the square root, plus rsqrtf (specified to 1 ulp; 2 allowed)
    rho = (0.5 * (Lr + 5) + 4) * U
    within(rstd, r64, rho * r64, "LayerNorm rstd")
    g64, b64 = gamma[:Cr].double(), beta[:Cr].double()
    xh = (xr - mu[:, None]) * r64[:, None]
    ref = xh * g64 + b64
    bound = ulp_bf16(ref) + g64.abs() * (dmu[:, None] * r64[:, None] + xh.abs() * rho) + 4 * U * ((xh * g64).abs() + b64.abs())
    within(y[:, :Cr], ref, bound, "LayerNorm y")
    assert not bool(y[:, Cr:].float().ne(0).any()), "padded y columns must be exactly zero"

    nb = L.lib.pk_ln_bwd_blocks(rows)
    # the reference is fed the statistics the kernel saved
    mk, rk = mean.double()[:, None], rstd.double()[:, None]
    xh = (xr - mk) * rk
    gy = dy[:, :Cr].double()
    gh = gy * g64
    m1, m2 = gh.mean(1, keepdim=True), (gh * xh).mean(1, keepdim=True)
    core = rk * (gh - m1 - xh * m2)
    d1 = (Lr + 2) * U * gh.abs().sum(1, keepdim=True) / Cr
    d2 = (Lr + 4) * U * (gh * xh).abs().sum(1, keepdim=True) / Cr
    ecore = rk * (4 * U * (gh.abs() + m1.abs() + (xh * m2).abs()) + d1 + xh.abs() * d2) + 2 * U * core.abs()
    Lc = chain(rows, nb, 256 // lanes) + 4
    dgs = []
    for with_res in (False, True):
        dx = nan_like(x)
        part = torch.full((nb, 2, C), NAN, device=DEV)
        dg, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
        call(L, "pk_layernorm_bwd", dy, x, mean, rstd, gamma, dres if with_res else None, dx, part, dg, db, rows, C, Cr)
        ref = core + (dres[:, :Cr].double() if with_res else 0)
        bound = ulp_bf16(ref) + ecore + (2 * U * dres[:, :Cr].double().abs() if with_res else 0)
        within(dx[:, :Cr], ref, bound, f"LayerNorm dx (dresidual {with_res})")
        assert not bool(dx[:, Cr:].float().ne(0).any()), "padded dx columns must be exactly zero"
        tg, tb = gy * xh, gy
        within(dg[:Cr], tg.sum(0), Lc * U * tg.abs().sum(0), "LayerNorm dgamma")
        within(db[:Cr], tb.sum(0), Lc * U * tb.abs().sum(0), "LayerNorm dbeta")
        assert not bool(dg[Cr:].ne(0).any() or db[Cr:].ne(0).any()), "padded dgamma / dbeta entries must be exactly zero"
        dgs.append(torch.cat([dg, db]))
    assert torch.equal(dgs[0], dgs[1]), "dgamma / dbeta depend on dresidual"


# ================================================================================================ generic reductions
@pytest.mark.parametrize("nb", [1, 63, 64, 65, 255, 256, 257, 1024])
def test_sum_partials_vs_fp64(L, nb):
    K, stride = 37, 45
    g = gen(nb)
    s = 10.0 ** (torch.rand(K, generator=g, device=DEV) * 4 - 2)
    off = (torch.rand(K, generator=g, device=DEV) * 2 - 1) * 8 * s
    part = torch.full((nb, stride), NAN, device=DEV)              # the columns past K must not be read
    part[:, :K] = torch.randn(nb, K, generator=g, device=DEV) * s + off
    scale = float(np.float32(0.37))
    out = torch.full((K + 3,), NAN, device=DEV)
    call(L, "pk_sum_partials", part, nb, K, stride, out, scale, 0)
    torch.cuda.synchronize()
    p64 = part[:, :K].double()
    ref = p64.sum(0) * scale
    # float64 sum (its order: 2^-50 of the magnitudes) rounded once to fp32, then one fp32 product: within 2 fp32 ulp
    within(out[:K], ref, 2 * ulp_f32(ref) + 2.0 ** -50 * p64.abs().sum(0) * scale, "pk_sum_partials")
    assert bool(torch.isnan(out[K:]).all()), "pk_sum_partials wrote past K"
    old = torch.randn(K + 3, generator=g, device=DEV) * s.repeat(2)[:K + 3]
    acc = old.clone()
    call(L, "pk_sum_partials", part, nb, K, stride, acc, scale, 1)
    torch.cuda.synchronize()
    assert torch.equal(acc[:K], old[:K] + out[:K]), "accumulate: not the fp32 sum of the old value and the scaled partial sum"
    assert torch.equal(acc[K:], old[K:])


@pytest.mark.parametrize("N", [64, 40])
def test_colsum_rowmap_row_scale_many_blocks(L, N):
    rows, rps = 196608, 3072
    gt = chan_data(rows, N, N)
    g = gen(N + 1)
    rowmap = torch.randperm(rows, generator=g, device=DEV).to(torch.int32)
    rowmap[torch.rand(rows, generator=g, device=DEV) < 0.1] = -1                  # -1 rows are skipped
    row_scale = (10.0 ** (torch.rand(rows // rps, generator=g, device=DEV) * 2 - 1)).float()
    nb = L.lib.pk_ln_bwd_blocks(rows)
    part, out = torch.full((nb, N), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    call(L, "pk_colsum_bf16", gt, rowmap, row_scale, rps, part, out, rows, N)
    torch.cuda.synchronize()
    src = rowmap.long()
    src = src[src >= 0]
    terms = gt.double()[src] * row_scale.double()[src // rps][:, None]
    Lc = chain(rows, nb, 256 // (N // 8)) + 2                           # + the product rounding and the final rounding
    within(out, terms.sum(0), Lc * U * terms.abs().sum(0), "pk_colsum_bf16")


# ================================================================================================ one training layer end to end
def test_conv_bn_act_training_at_hrnet_w32_branch0_size(L):
    """nnops.conv_bn_act(training=True) at HRNet-W32's branch-0 BasicBlock shape (32 -> 32 3x3, B = 32, 96x72, + residual, ReLU): k_conv3h
    statistics -> the large BatchNorm paths -> dgrad / wgrad, against a float64 CPU reference with the kernel's bf16 storage rounding.
    Bars of the 240-row test_conv_bn_act_function."""
    from conftest import rel_err
    from oracle import nets as onet
    from infantposeestimation_gaussianbias_amd import nnops
    B, H, W, C = 32, 96, 72, 32
    torch.manual_seed(21)
    conv, bn = torch.nn.Conv2d(C, C, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(C)
    q = lambda t: t.to(BF).float()      # noqa: E731
    with torch.no_grad():
        conv.weight.copy_(q(conv.weight * 2))
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.2)
        bn.running_mean.copy_(torch.randn(C) * 0.1)
        bn.running_var.copy_(torch.rand(C) + 0.5)
    x, r, gy = q(torch.randn(B, C, H, W)), q(torch.randn(B, C, H, W)), q(torch.randn(B, C, H, W))
    P = {"c.weight": conv.weight.detach().double().requires_grad_(True), "b.weight": bn.weight.detach().double().requires_grad_(True),
         "b.bias": bn.bias.detach().double().requires_grad_(True), "b.running_mean": bn.running_mean.double(),
         "b.running_var": bn.running_var.double(), "b.num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    ctx = onet.Ctx(train=True, q=onet.bf16_storage)
    xr, rr = x.double().requires_grad_(True), r.double().requires_grad_(True)
    y_ref = torch.relu(onet.batchnorm(onet.conv(xr, P, "c"), P, "b", ctx) + rr)
    y_ref.backward(gy.double())
    onet.apply_bn_updates(P, ctx)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c, self.b = conv, bn
    m = Holder().to(DEV).train()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV, BF)                  # noqa: E731
    nchw = lambda t: t.detach().float().cpu().permute(0, 3, 1, 2).double()           # noqa: E731
    with nnops.use_weights(m):
        xd, rd = nhwc(x).requires_grad_(True), nhwc(r).requires_grad_(True)
        y = nnops.conv_bn_act(xd, m.c, m.b, True, rd, True)
        y.backward(nhwc(gy))
    torch.cuda.synchronize()
    e = lambda a, b: rel_err(a.detach().double().cpu().numpy(), b.detach().numpy())  # noqa: E731
    assert e(nchw(y), y_ref) < 8e-3
    rep = {"gx": e(nchw(xd.grad), xr.grad), "gw": e(m.c.weight.grad, P["c.weight"].grad), "ggamma": e(m.b.weight.grad, P["b.weight"].grad),
           "gbeta": e(m.b.bias.grad, P["b.bias"].grad), "gres": e(nchw(rd.grad), rr.grad)}
    print("conv_bn_act at 221 184 rows vs float64", {k: round(v, 5) for k, v in rep.items()})
    assert all(v < 2e-2 for v in rep.values()), rep
    assert e(m.b.running_mean, P["b.running_mean"]) < 5e-3 and e(m.b.running_var, P["b.running_var"]) < 5e-3
    assert int(m.b.num_batches_tracked) == 1
