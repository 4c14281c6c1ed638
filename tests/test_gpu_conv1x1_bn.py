"""GPU tests (`-m gpu`) of pk_conv1x1_bn.hip: the 64 -> 256 1x1 convolution recomputed inside the BatchNorm passes instead of stored.

The row threshold of the route is lowered to 1 and the grid capped at 3 workgroups (a workgroup then walks several 128-row tiles, a wave
of the backward reduce several partial rows), rows
M in {1, 127, 128, 129, 260, 1000}: below, at and above a tile, a wave's 32 rows cut, more tiles than workgroups.  Every 256-channel
buffer a kernel writes has a guard region behind it that must stay as it was.  The references are the stored-raw path the route replaces:
pk_conv2d_nhwc (+ statistics), pk_bn_finalize, pk_bn_act, pk_bn_bwd, computed once per M and shared.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CIN, COUT = 64, 256
ROWS = (1, 127, 128, 129, 260, 1000)
GUARD = 4096          # elements behind every output


@pytest.fixture(autouse=True)
def _route(monkeypatch):
    monkeypatch.setenv("PK_CONV1X1_BN_MIN_ROWS", "1")
    monkeypatch.setenv("PK_CONV1X1_BN_MAX_GRID", "3")


def _lib():
    from infantposeestimation_gaussianbias_amd import _lib as L
    return L


def call(name, *a):
    L = _lib()
    L.call(name, *a, L.stream_ptr())


class Guarded:
    """A tensor with GUARD elements of a fixed pattern behind it."""

    def __init__(self, n, dtype):
        self.full = torch.empty(n + GUARD, dtype=dtype, device=DEV)
        g = torch.arange(GUARD, device=DEV) % 251 + 1
        self.full[n:] = g.to(dtype)
        self.want = self.full[n:].clone()
        self.t = self.full[:n]
        if dtype.is_floating_point:
            self.t.fill_(float("nan"))
        else:
            self.t.fill_(0xA5)

    def intact(self):
        return torch.equal(self.full[self.t.numel():], self.want)


def ordered(t):
    """bf16 bit patterns as integers in value order (-0 and +0 coincide): a difference of 1 is one ulp"""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


def within_one_ulp(a, b):
    """every element at most one bf16 ulp apart -- or, where a difference cancels down to a tiny value whose ulp is below fp32 rounding of the
    terms it came from, within 1e-6 of the largest reference magnitude"""
    d = (ordered(a) - ordered(b)).abs() <= 1
    tiny = (a.float() - b.float()).abs() <= 1e-6 * float(b.float().abs().max())
    return bool((d | tiny).all())


def rnd(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def finalize(part, M, gamma, beta):
    """pk_bn_finalize on partial statistics -> dict of scale, shift, mean, rstd, running_mean, running_var"""
    o = {k: torch.empty(COUT, dtype=F32, device=DEV) for k in ("scale", "shift", "mean", "rstd")}
    o["running_mean"] = torch.linspace(-0.5, 0.5, COUT, device=DEV)
    o["running_var"] = torch.linspace(0.5, 1.5, COUT, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    call("pk_bn_finalize", part, part.shape[0], COUT, M, gamma, beta, o["running_mean"], o["running_var"], nbt, 0.1, 1e-5, o["scale"], o["shift"],
         o["mean"], o["rstd"])
    assert int(nbt) == 1
    return o


@functools.lru_cache(maxsize=None)
def problem(M):
    """Inputs and the stored-raw references of one row count (computed once, never modified)."""
    L = _lib().lib
    p = dict(M=M)
    p["x"] = rnd(M, CIN, seed=100 + M)
    p["w"] = rnd(COUT, 1, CIN, seed=7, scale=0.25)
    p["gamma"] = (torch.rand(COUT, generator=torch.Generator().manual_seed(8)) + 0.5).to(DEV)
    p["beta"] = (torch.randn(COUT, generator=torch.Generator().manual_seed(9)) * 0.2).to(DEV)
    p["res"] = rnd(M, COUT, seed=200 + M)
    p["dy"] = rnd(M, COUT, seed=300 + M)
    raw = torch.empty(M, COUT, dtype=BF, device=DEV)
    part = torch.empty(L.pk_conv_stats_rows(1, M, 1, CIN, COUT, 1, 1, M, 1), 2, COUT, dtype=F32, device=DEV)
    call("pk_conv2d_nhwc", p["x"], p["w"], raw, part, None, 1, M, 1, CIN, COUT, 1, 1, 0, M, 1, 0, 0, None)
    p["raw"], p["part"] = raw, part
    p["bn"] = finalize(part, M, p["gamma"], p["beta"])
    # forward references: pk_bn_act on the stored raw, one per (relu, residual); the ReLU cases keep their bit masks for the backward tests
    p["fwd"] = {}
    for relu, res in ((1, True), (1, False), (0, False)):
        y = torch.empty(M, COUT, dtype=BF, device=DEV)
        mask = torch.empty(M * COUT // 8, dtype=torch.uint8, device=DEV)
        call("pk_bn_act", raw, p["bn"]["scale"], p["bn"]["shift"], p["res"] if res else None, y, M, COUT, relu, mask)
        p["fwd"][(relu, res)] = (y, mask)
    torch.cuda.synchronize()
    return p


def bn_bwd_reference(p, relu, with_dres):
    """pk_bn_bwd on the stored raw -> draw, dres, sums [2][C] (what it wrote: the `sums` buffer in its large-tensor form, dbeta | dgamma -- the same
    values -- in the small-tensor form, which folds the sum into its apply kernel and leaves `sums` alone)"""
    L, M = _lib().lib, p["M"]
    mask = p["fwd"][(1, False)][1] if relu else None
    part = torch.empty(L.pk_bn_bwd_blocks(M), 2, COUT, dtype=F32, device=DEV)
    sums = torch.full((2 * COUT,), float("nan"), dtype=F32, device=DEV)
    dgamma, dbeta = torch.empty(COUT, dtype=F32, device=DEV), torch.empty(COUT, dtype=F32, device=DEV)
    draw = torch.empty(M, COUT, dtype=BF, device=DEV)
    dres = torch.empty(M, COUT, dtype=BF, device=DEV) if with_dres else None
    call("pk_bn_bwd", p["dy"], None, p["raw"], p["bn"]["mean"], p["bn"]["rstd"], p["gamma"], part, sums, dgamma, dbeta, draw, dres, M, COUT, relu, mask)
    torch.cuda.synchronize()
    wrote_sums = not bool(torch.isnan(sums).any())
    if not wrote_sums:
        sums = torch.cat([dbeta, dgamma])
    else:
        assert torch.equal(sums, torch.cat([dbeta, dgamma]))
    bn_bwd_reference.partial = part          # the reduce stage's partial rows of the call just made
    return draw, dres, sums, wrote_sums, mask


# ------------------------------------------------------------------------------------------------ 1. the recomputed raw
@pytest.mark.parametrize("M", ROWS)
def test_recomputed_raw_is_the_stored_raw(M):
    """Apply pass with scale = 1, shift = 0, no residual, no ReLU: bit for bit pk_conv2d_nhwc's output (same MFMA, same k order)."""
    p = problem(M)
    y = Guarded(M * COUT, BF)
    one, zero = torch.ones(COUT, device=DEV), torch.zeros(COUT, device=DEV)
    call("pk_conv1x1_bn_act", p["x"], p["w"], one, zero, None, y.t, 0, None, M, CIN, COUT)
    torch.cuda.synchronize()
    assert y.intact()
    assert torch.equal(y.t.view(M, COUT).view(torch.int16), p["raw"].view(torch.int16))


# ------------------------------------------------------------------------------------------------ 2. statistics
@pytest.mark.parametrize("M", ROWS)
def test_statistics_pass_feeds_bn_finalize(M):
    """The statistics-only pass through pk_bn_finalize against pk_conv2d_nhwc's partial sums through the same call: mean, rstd and the
    running statistics to 1e-5 (another summation order of the same fp32 accumulators at most)."""
    L = _lib().lib
    p = problem(M)
    tiles = L.pk_conv1x1_stats_rows(M)
    assert tiles == (M + 127) // 128
    part = Guarded(tiles * 2 * COUT, F32)
    call("pk_conv1x1_stats", p["x"], p["w"], part.t, M, CIN, COUT)
    torch.cuda.synchronize()
    assert part.intact() and bool(torch.isfinite(part.t).all())
    got = finalize(part.t.view(tiles, 2, COUT), M, p["gamma"], p["beta"])
    torch.cuda.synchronize()
    rep = {k: rel_err(got[k].cpu().numpy(), p["bn"][k].cpu().numpy()) for k in ("mean", "rstd", "running_mean", "running_var")}
    print(f"M={M} statistics vs conv epilogue", rep)
    assert all(v <= 1e-5 for v in rep.values()), rep


# ------------------------------------------------------------------------------------------------ 3. forward apply
@pytest.mark.parametrize("relu,res", [(1, True), (1, False), (0, False)])
@pytest.mark.parametrize("M", ROWS)
def test_forward_apply_equals_bn_act_on_the_stored_raw(M, relu, res):
    """Same scale / shift arrays: y and the ReLU bit mask bit-equal to pk_bn_act on the stored raw."""
    p = problem(M)
    y, mask = Guarded(M * COUT, BF), Guarded(M * COUT // 8, torch.uint8)
    call("pk_conv1x1_bn_act", p["x"], p["w"], p["bn"]["scale"], p["bn"]["shift"], p["res"] if res else None, y.t, relu, mask.t, M, CIN, COUT)
    torch.cuda.synchronize()
    assert y.intact() and mask.intact()
    y_ref, mask_ref = p["fwd"][(relu, res)]
    assert torch.equal(y.t.view(M, COUT).view(torch.int16), y_ref.view(torch.int16))
    assert torch.equal(mask.t, mask_ref)


# ------------------------------------------------------------------------------------------------ 4. backward
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("M", ROWS + (32768 + 129,))
def test_backward_reduce_against_float64(M, relu):
    """Reduce-stage partial rows, summed, against a float64 sum of the same terms g and g * xhat (g = dy under the ReLU bits, xhat from the
    stored raw): 1e-5 of the sum of |term| per channel."""
    L = _lib().lib
    p = problem(M)
    nb = L.pk_conv1x1_bn_bwd_rows(M)
    assert nb == L.pk_bn_bwd_blocks(M)          # pk_bn_bwd's own split of the rows, one wave per partial row
    mask = p["fwd"][(1, False)][1] if relu else None
    part = Guarded(nb * 2 * COUT, F32)
    call("pk_conv1x1_bn_bwd_reduce", p["dy"], p["x"], p["w"], p["bn"]["mean"], p["bn"]["rstd"], part.t, M, CIN, COUT, relu, mask)
    torch.cuda.synchronize()
    assert part.intact()
    # ... and the same additions in the same order: the partial rows are k_bn_bwd_reduce's, bit for bit
    bn_bwd_reference(p, relu, False)
    assert torch.equal(part.t.view(nb, 2, COUT).view(torch.int32), bn_bwd_reference.partial.view(torch.int32))
    got = part.t.view(nb, 2, COUT).double().sum(0).cpu()
    g = p["dy"].double().cpu()
    if relu:
        bits = ((mask.cpu().view(M, COUT // 8, 1).int() >> torch.arange(8).view(1, 1, 8)) & 1).reshape(M, COUT)
        g = g * bits.double()
    xhat = (p["raw"].double().cpu() - p["bn"]["mean"].double().cpu()) * p["bn"]["rstd"].double().cpu()
    for k, term in enumerate((g, g * xhat)):
        bound = 1e-5 * term.abs().sum(0)
        diff = (got[k] - term.sum(0)).abs()
        print(f"M={M} relu={relu} sum {k}: worst diff / bound = {float((diff / bound.clamp_min(1e-30)).max()):.3g}")
        assert bool((diff <= bound).all())


def _apply_stage(p, sums, relu, with_dres, mask):
    M = p["M"]
    draw = Guarded(M * COUT, BF)
    dres = Guarded(M * COUT, BF) if with_dres else None
    inv = ctypes.c_float(float(np.float32(1.0) / np.float32(M)))
    call("pk_conv1x1_bn_bwd_apply", p["dy"], p["x"], p["w"], p["bn"]["mean"], p["bn"]["rstd"], p["gamma"], sums, inv, draw.t,
         dres.t if with_dres else None, M, CIN, COUT, relu, mask)
    torch.cuda.synchronize()
    assert draw.intact() and (dres is None or dres.intact())
    return draw.t.view(M, COUT), (dres.t.view(M, COUT) if with_dres else None)


def _apply_formula(p, sums, relu, mask):
    """k_bn_bwd_apply's arithmetic, one rounded fp32 operation per step, on the stored raw."""
    M = p["M"]
    g = p["dy"].float()
    if relu:
        bits = ((mask.view(M, COUT // 8, 1).int() >> torch.arange(8, device=DEV).view(1, 1, 8)) & 1).reshape(M, COUT)
        g = torch.where(bits.bool(), g, torch.zeros_like(g))
    inv = torch.tensor(float(np.float32(1.0) / np.float32(M)), dtype=F32, device=DEV)
    mean, rstd, gamma = p["bn"]["mean"], p["bn"]["rstd"], p["gamma"]
    xh = (p["raw"].float() - mean) * rstd
    t = g - sums[:COUT] * inv
    t = t - (xh * sums[COUT:]) * inv
    return ((gamma * rstd) * t).to(BF), g.to(BF)


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("M", ROWS + (32768 + 129,))
def test_backward_apply_equals_bn_bwd(M, relu, with_dres):
    """The apply stage on the sums pk_bn_bwd wrote for the same problem: draw and dresidual bit-equal to pk_bn_bwd's.

    pk_bn_bwd writes a `sums` buffer, and evaluates k_bn_bwd_apply's expression, only in its large-tensor form (rows > 32 768: the form the
    route replaces in the network).  That is the 32 897-row case: bit-equal to pk_bn_bwd, outright.  At the small row counts pk_bn_bwd takes
    k_bn_bwd_apply_fin, which leaves `sums` unwritten (the same two sums go to dbeta | dgamma, taken from there) and multiplies
    xhat * (sum * inv_count) where k_bn_bwd_apply multiplies (xhat * sum) * inv_count: one fp32 rounding apart before the bf16 store.
    There the new kernel must be bit-equal to k_bn_bwd_apply's expression evaluated one rounded fp32 operation at a time on the stored
    raw, dresidual bit-equal to pk_bn_bwd's, and draw within one bf16 ulp of pk_bn_bwd's small-tensor form."""
    p = problem(M)
    draw_ref, dres_ref, sums, wrote_sums, mask = bn_bwd_reference(p, relu, with_dres)
    assert wrote_sums == (M > 32768)
    draw, dres = _apply_stage(p, sums, relu, with_dres, mask)
    if with_dres:
        assert torch.equal(dres.view(torch.int16), dres_ref.view(torch.int16))
    if wrote_sums:
        assert torch.equal(draw.view(torch.int16), draw_ref.view(torch.int16))
        return
    want, _ = _apply_formula(p, sums, relu, mask)
    assert torch.equal(draw.view(torch.int16), want.view(torch.int16))
    assert within_one_ulp(draw, draw_ref), "more than one bf16 ulp from pk_bn_bwd's small-tensor form"


@pytest.mark.parametrize("M", (260, 32768 + 129))
def test_composed_backward_is_reduce_sum_apply(M):
    """pk_conv1x1_bn_bwd = reduce + fixed-order sum + apply: dbeta | dgamma equal its `sums`, which are the sum of its partial rows (1e-6);
    dresidual bit-equal to pk_bn_bwd's; in pk_bn_bwd's large-tensor form (32 897 rows) sums and draw are bit-equal to pk_bn_bwd's as well
    (same partial rows, same sum kernel, same apply expression), at 260 rows draw is within the 8e-3 of one bf16 store of its small-tensor
    form (sums combined in double there); two runs give identical bytes."""
    L = _lib().lib
    p = problem(M)
    draw_ref, dres_ref, sums_ref, _, mask = bn_bwd_reference(p, 1, True)
    outs = []
    for _ in range(2):
        part = torch.empty(L.pk_conv1x1_bn_bwd_rows(M), 2, COUT, dtype=F32, device=DEV)
        sums, dgamma, dbeta = (torch.empty(n, dtype=F32, device=DEV) for n in (2 * COUT, COUT, COUT))
        draw, dres = Guarded(M * COUT, BF), Guarded(M * COUT, BF)
        call("pk_conv1x1_bn_bwd", p["dy"], p["x"], p["w"], p["bn"]["mean"], p["bn"]["rstd"], p["gamma"], part, sums, dgamma, dbeta, draw.t, dres.t,
             M, CIN, COUT, 1, mask)
        torch.cuda.synchronize()
        assert draw.intact() and dres.intact()
        assert torch.equal(sums, torch.cat([dbeta, dgamma]))
        assert rel_err(sums.cpu().numpy(), part.double().sum(0).view(-1).cpu().numpy()) <= 1e-6
        outs.append((sums, draw.t.view(M, COUT), dres.t.view(M, COUT)))
    for u, v in zip(*outs):
        assert torch.equal(u.view(-1).view(torch.int16 if u.dtype == BF else torch.int32), v.view(-1).view(torch.int16 if v.dtype == BF else torch.int32))
    sums, draw, dres = outs[0]
    assert torch.equal(dres.view(torch.int16), dres_ref.view(torch.int16))
    if M > 32768:
        assert torch.equal(sums.view(torch.int32), sums_ref.view(torch.int32))
        assert torch.equal(draw.view(torch.int16), draw_ref.view(torch.int16))
    else:
        assert rel_err(draw.float().cpu().numpy(), draw_ref.float().cpu().numpy()) < 8e-3


# ------------------------------------------------------------------------------------------------ 5. op level
class Holder(torch.nn.Module):
    def __init__(self, **mods):
        super().__init__()
        for k, v in mods.items():
            setattr(self, k, v)


def _nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(DEV, BF)


def _nchw(x_nhwc):
    return x_nhwc.detach().float().cpu().permute(0, 3, 1, 2)


def _err(a, b):
    return rel_err(a.detach().float().cpu().numpy(), b.detach().float().cpu().numpy())


def test_op_level_route_on_and_off(monkeypatch):
    """nnops.conv_bn_act on Conv2d(64, 256, 1) + BatchNorm + residual + ReLU, B = 2 at 16x12 (384 rows), with the route on and off: both
    within the bars of test_gpu_network_ops.py::test_conv_bn_act_function (restated: y 8e-3, gradients 2e-2, running statistics 5e-3 against
    the storage-aware oracle); y of the two routes at most one bf16 ulp apart (statistics that agree to 1e-5 move no value further); no
    tensor of raw's shape among the tensors the new route saves for backward."""
    from infantposeestimation_gaussianbias_amd import nnops as N
    from oracle import nets as onet
    q = lambda t: t.to(BF).float()      # noqa: E731
    torch.manual_seed(5)
    conv, bn = torch.nn.Conv2d(CIN, COUT, 1, 1, 0, bias=False), torch.nn.BatchNorm2d(COUT)
    with torch.no_grad():
        conv.weight.copy_(q(conv.weight * 2))
        bn.weight.copy_(torch.rand(COUT) + 0.5)
        bn.bias.copy_(torch.randn(COUT) * 0.2)
        bn.running_mean.copy_(torch.randn(COUT) * 0.1)
        bn.running_var.copy_(torch.rand(COUT) + 0.5)
    g = torch.Generator().manual_seed(6)
    x, r, gy = (q(torch.randn(2, c, 16, 12, generator=g)) for c in (CIN, COUT, COUT))
    P = {"c.weight": conv.weight.detach().clone().requires_grad_(True), "b.weight": bn.weight.detach().clone().requires_grad_(True),
         "b.bias": bn.bias.detach().clone().requires_grad_(True), "b.running_mean": bn.running_mean.clone(), "b.running_var": bn.running_var.clone(),
         "b.num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    ctx = onet.Ctx(train=True, q=onet.bf16_storage)
    xr, rr = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    y_ref = torch.relu(onet.batchnorm(onet.conv(xr, P, "c"), P, "b", ctx) + rr)
    y_ref.backward(gy)
    onet.apply_bn_updates(P, ctx)
    ys = {}
    for route in ("1", "0"):
        monkeypatch.setenv("PK_CONV1X1_BN", route)
        assert _lib().lib.pk_conv1x1_bn_supported(2 * 16 * 12, CIN, COUT) == int(route)
        m = Holder(c=copy.deepcopy(conv), b=copy.deepcopy(bn)).to(DEV).train()
        with N.use_weights(m):
            xd, rd = _nhwc(x).requires_grad_(True), _nhwc(r).requires_grad_(True)
            y = N.conv_bn_act(xd, m.c, m.b, True, rd, True)
            saved = [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None]
            big = [s for s in saved if int(np.prod(s)) == y.numel()]
            if route == "1":
                assert not big, f"a tensor of raw's size is saved on the recomputing route: {saved}"
            else:
                assert big, "the stored-raw route no longer saves raw: the check above checks nothing"
            assert _err(_nchw(y), y_ref) < 8e-3
            y.backward(_nhwc(gy))
            rep = {"gx": _err(_nchw(xd.grad), xr.grad), "gw": _err(m.c.weight.grad, P["c.weight"].grad),
                   "ggamma": _err(m.b.weight.grad, P["b.weight"].grad), "gbeta": _err(m.b.bias.grad, P["b.bias"].grad),
                   "gres": _err(_nchw(rd.grad), rr.grad)}
            print(f"route {route}: conv_bn_act vs storage-aware oracle", {k: round(v, 4) for k, v in rep.items()})
            assert all(v < 2e-2 for v in rep.values()), rep
            assert _err(m.b.running_mean, P["b.running_mean"]) < 5e-3
            assert _err(m.b.running_var, P["b.running_var"]) < 5e-3
            assert int(m.b.num_batches_tracked) == 1
        ys[route] = y.detach()
    assert int((ordered(ys["1"]) - ordered(ys["0"])).abs().max()) <= 1, "y of the two routes more than one bf16 ulp apart"
