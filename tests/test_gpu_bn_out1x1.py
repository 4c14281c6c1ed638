"""GPU tests (`-m gpu`) of pk_bn_out1x1.hip: BatchNorm + ReLU + the 1x1 output conv of a fusion-head branch in one forward pass, and
BatchNorm backward with the output conv's data gradient dt recomputed instead of stored, against the stored route it replaces
(PK_BN_OUT1X1=0: pk_bn_act / pk_bn_train_fwd, pk_conv2d_nhwc, pk_bn_bwd) on the same inputs.

The row threshold is lowered to 1; every case runs with the default grid and with PK_BN_OUT1X1_MAX_GRID=1 (one workgroup walks every tile
and every partial row).  Shapes (B, H, W): (2, 9, 7) = 126 rows, less than one 128-row tile and no multiple of 8, 16 or 32; (3, 16, 11) =
528 rows, four tiles plus 16 rows, 17 partial rows of 32 with a ragged last one.  Branch forms (hidden width C, outputs N): (256, 17),
(256, 34), (128, 17) with softplus.  Everything is required bit for bit: the maps, the activated tensor, the ReLU bits, the running
statistics, the partial rows, dgamma, dbeta, draw, the 3x3 conv's dx and dW and the output conv's dW and db (its weight gradient is the
stored route's own launch on the same tensors), and with them one whole training step of the full model.

pk_bn_bwd has two forms (32 768 rows and fewer: the partial rows summed in double inside its apply kernel; above: summed by the partial-sum
kernel, another apply expression); the shapes above take the first, the network's 196 608 rows the second, which the kernel-level case at
32 897 rows (33 rows per partial row: blocks that start at any row) pins the same way.
"""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = ((2, 9, 7), (3, 16, 11))
FORMS = ((256, 17, False), (256, 34, False), (128, 17, True))
GRIDS = (None, "1")
GUARD = 4096
ENV = ("PK_BN_OUT1X1", "PK_BN_OUT1X1_MIN_ROWS", "PK_BN_OUT1X1_MAX_GRID")


def _lib():
    from infantposeestimation_gaussianbias_amd import _lib as L
    return L


def call(name, *a):
    L = _lib()
    L.call(name, *a, L.stream_ptr())


def _route(mp, on, grid=None):
    for k in ENV:
        mp.delenv(k, raising=False)
    mp.setenv("PK_BN_OUT1X1_MIN_ROWS", "1")
    if not on:
        mp.setenv("PK_BN_OUT1X1", "0")
    if grid:
        mp.setenv("PK_BN_OUT1X1_MAX_GRID", grid)


class Guarded:
    """A tensor with GUARD elements of a fixed pattern behind it."""

    def __init__(self, n, dtype):
        self.full = torch.empty(n + GUARD, dtype=dtype, device=DEV)
        self.full[n:] = (torch.arange(GUARD, device=DEV) % 251 + 1).to(dtype)
        self.want = self.full[n:].clone()
        self.t = self.full[:n]
        if dtype.is_floating_point:
            self.t.fill_(float("nan"))
        else:
            self.t.fill_(0xA5)

    def intact(self):
        return torch.equal(self.full[self.t.numel():], self.want)


def bits(t):
    return t.contiguous().view(-1).view({BF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}[t.dtype])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def up8(n):
    return -(-n // 8) * 8


# ------------------------------------------------------------------------------------------------ 1. the kernels against the stored calls
@functools.lru_cache(maxsize=None)
def problem(B, H, W, C, N, softplus):
    """Inputs and the stored route's results of one case, computed once and never modified."""
    M, N8 = B * H * W, up8(N)
    seed = 1000 * C + 10 * N + M
    p = dict(M=M, N8=N8)
    p["raw"] = rnd(M, C, seed=seed, dtype=BF)
    p["scale"] = (torch.rand(C, generator=torch.Generator().manual_seed(seed + 1)) + 0.5).to(DEV)
    p["shift"] = rnd(C, seed=seed + 2, scale=0.3)
    p["mean"] = rnd(C, seed=seed + 3, scale=0.2)
    p["rstd"] = (torch.rand(C, generator=torch.Generator().manual_seed(seed + 4)) + 0.5).to(DEV)
    p["gamma"] = (torch.rand(C, generator=torch.Generator().manual_seed(seed + 5)) + 0.5).to(DEV)
    w = rnd(N, C, seed=seed + 6, scale=0.1)
    p["bias"] = rnd(N, seed=seed + 7, scale=0.5)
    p["dout"] = rnd(B, N, H, W, seed=seed + 8)
    p["wf"] = w.to(BF).view(N, 1, C).contiguous()                         # pk_pack_weights mode 0
    wd = torch.zeros(C, 1, N8, dtype=BF, device=DEV)                      # mode 1 (one tap): [C][N padded to 8]
    wd[:, 0, :N] = w.t().to(BF)
    p["wd"] = wd
    # forward: pk_bn_act, then the 1x1 conv to fp32 planes with bias (softplus)
    t = torch.empty(M, C, dtype=BF, device=DEV)
    mask = torch.empty(M * C // 8, dtype=torch.uint8, device=DEV)
    call("pk_bn_act", p["raw"], p["scale"], p["shift"], None, t, M, C, 1, mask)
    out = torch.empty(B, N, H, W, dtype=F32, device=DEV)
    call("pk_conv2d_nhwc", t, p["wf"], out, None, p["bias"], B, H, W, C, N, 1, 1, 0, H, W, 2 if softplus else 0, 2, None)
    p["t"], p["mask"], p["out"] = t, mask, out
    # backward: converter (8-aligned channels), 1x1 data gradient, pk_bn_bwd
    g = torch.empty(M, N8, dtype=BF, device=DEV)
    call("pk_nchw_f32_to_nhwc_bf16", p["dout"], out if softplus else None, g, B, N, H, W, N8)
    dt = torch.empty(M, C, dtype=BF, device=DEV)
    call("pk_conv2d_nhwc", g, wd, dt, None, None, B, H, W, N8, C, 1, 1, 0, H, W, 0, 0, None)
    L = _lib().lib
    nb = L.pk_bn_bwd_blocks(M)
    part = torch.empty(nb, 2, C, dtype=F32, device=DEV)
    sums, dgamma, dbeta = (torch.empty(n, dtype=F32, device=DEV) for n in (2 * C, C, C))
    draw = torch.empty(M, C, dtype=BF, device=DEV)
    call("pk_bn_bwd", dt, None, p["raw"], p["mean"], p["rstd"], p["gamma"], part, sums, dgamma, dbeta, draw, None, M, C, 1, mask)
    torch.cuda.synchronize()
    p.update(g=g, dt=dt, part=part, dgamma=dgamma, dbeta=dbeta, draw=draw)
    return p


def _kernel_case(B, H, W, C, N, softplus, grid, monkeypatch):
    L = _lib().lib
    p = problem(B, H, W, C, N, softplus)
    M = p["M"]
    _route(monkeypatch, True, grid)
    assert L.pk_bn_out1x1_supported(M, C, N) == 1
    tag = f"rows={M} C={C} N={N} grid={grid or 'default'}"
    # ---- forward
    out, mask, t = Guarded(B * N * H * W, F32), Guarded(M * C // 8, torch.uint8), Guarded(M * C, BF)
    call("pk_bn_out1x1_fwd", p["raw"], p["scale"], p["shift"], p["wf"], p["bias"], t.t, out.t, mask.t, M, C, N, H * W, 1 if softplus else 0)
    torch.cuda.synchronize()
    assert out.intact() and mask.intact() and t.intact()
    assert same(t.t, p["t"].view(-1)), tag
    assert same(mask.t, p["mask"]), tag
    assert same(out.t, p["out"].view(-1)), tag
    # ---- backward, on the converter's output as the stored route makes it
    nb = L.pk_bn_bwd_blocks(M)
    part, draw = Guarded(nb * 2 * C, F32), Guarded(M * C, BF)
    sums, dgamma, dbeta = (torch.empty(n, dtype=F32, device=DEV) for n in (2 * C, C, C))
    call("pk_bn_out1x1_bwd", p["g"], p["raw"], p["mask"], p["wd"], p["mean"], p["rstd"], p["gamma"], part.t, sums, dgamma, dbeta, draw.t, M, C, N)
    torch.cuda.synchronize()
    assert part.intact() and draw.intact()
    assert same(part.t, p["part"].view(-1)), tag
    assert same(dgamma, p["dgamma"]) and same(dbeta, p["dbeta"]) and same(sums, torch.cat([p["dbeta"], p["dgamma"]])), tag
    assert same(draw.t, p["draw"].view(-1)), tag


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C,N,softplus", FORMS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_kernels_equal_the_stored_calls(B, H, W, C, N, softplus, grid, monkeypatch):
    _kernel_case(B, H, W, C, N, softplus, grid, monkeypatch)


@pytest.mark.parametrize("C,N,softplus", [(256, 17, False), (128, 17, True)])
def test_kernels_equal_the_stored_calls_in_the_large_tensor_form(C, N, softplus, monkeypatch):
    """32 897 rows: pk_bn_bwd's form above 32 768 rows, the one the network's head takes; 1024 partial rows of 33 rows."""
    _kernel_case(1, 32897, 1, C, N, softplus, None, monkeypatch)


# ------------------------------------------------------------------------------------------------ 2. the op
class Holder(torch.nn.Module):
    def __init__(self, **mods):
        super().__init__()
        for k, v in mods.items():
            setattr(self, k, v)


def _run_op(m0, x, dout, softplus, monkeypatch, on, grid=None):
    from infantposeestimation_gaussianbias_amd import nnops
    _route(monkeypatch, on, grid)
    m = copy.deepcopy(m0).to(DEV).train()
    with nnops.use_weights(m):
        xd = x.clone().requires_grad_(True)
        out = nnops.conv_bn_act_out(xd, m.c, m.b, m.o, softplus, True)
        assert ("_ConvBnActOut" in type(out.grad_fn).__name__) == on
        if on:
            t, mask = out.grad_fn.saved_tensors[2], out.grad_fn.saved_tensors[3]
        else:
            t, mask = out.grad_fn.saved_tensors[0], out.grad_fn.next_functions[0][0].saved_tensors[2]
        r = dict(out=out.detach().clone(), t=t.clone(), mask=mask.clone())
        out.backward(dout)
    torch.cuda.synchronize()
    r.update(dx=xd.grad, dw=m.c.weight.grad, dgamma=m.b.weight.grad, dbeta=m.b.bias.grad, ow=m.o.weight.grad, ob=m.o.bias.grad,
             rm=m.b.running_mean, rv=m.b.running_var, nbt=m.b.num_batches_tracked)
    return r


@pytest.mark.parametrize("C,N,softplus", FORMS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_op_fused_against_stored(B, H, W, C, N, softplus, monkeypatch):
    """nnops.conv_bn_act_out on Conv2d(16, C, 3) + BatchNorm + ReLU + Conv2d(C, N, 1): the route on (default grid, one workgroup) and off."""
    CIN = 16
    torch.manual_seed(3)
    m0 = Holder(c=torch.nn.Conv2d(CIN, C, 3, 1, 1, bias=False), b=torch.nn.BatchNorm2d(C), o=torch.nn.Conv2d(C, N, 1))
    with torch.no_grad():
        m0.b.weight.copy_(torch.rand(C) + 0.5)
        m0.b.bias.copy_(torch.randn(C) * 0.2)
        m0.b.running_mean.copy_(torch.randn(C) * 0.1)
        m0.b.running_var.copy_(torch.rand(C) + 0.5)
        m0.o.bias.copy_(torch.randn(N) * 0.3)
    x = rnd(B, H, W, CIN, seed=50 + B, dtype=BF)
    dout = rnd(B, N, H, W, seed=60 + B)
    stored = _run_op(m0, x, dout, softplus, monkeypatch, False)
    M = B * H * W
    for grid in GRIDS:
        tag = f"op rows={M} C={C} N={N} grid={grid or 'default'}"
        fused = _run_op(m0, x, dout, softplus, monkeypatch, True, grid)
        for k in ("out", "t", "mask", "rm", "rv", "nbt", "dgamma", "dbeta", "dx", "dw", "ow", "ob"):
            assert same(fused[k], stored[k]), (tag, k)


# ------------------------------------------------------------------------------------------------ 3. one training step of the full model
def test_trainer_step_fused_against_stored(monkeypatch):
    """HRFormer-small + fusion head, B = 4 at 128x96 (3 072 head rows): one step on the stored route puts the gradient sinks in place, then
    one forward + backward from those identical weights on either route.  Loss, every gradient and every BatchNorm buffer bit-equal."""
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    from infantposeestimation_gaussianbias_amd.models import build_model
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    batch = synthetic_batch(4, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=21)
    res = {}
    for on in (False, True):
        _route(monkeypatch, False)
        torch.manual_seed(0)
        model = build_model(cfg).to(DEV)
        model.backbone.drop_path_rate = 0.0
        tr = engine.Trainer(model, cfg, iters_per_epoch=2)
        tr.step(batch)
        _route(monkeypatch, on)
        out = tr._fwd_bwd(batch)
        torch.cuda.synchronize()
        res[on] = dict(flat=tr.opt.flat.clone(), loss=out["loss"].detach().clone().reshape(1), grad=tr.opt.grad.clone(),
                       grads={n: tr.opt.grad_view(i).clone() for i, n in enumerate(tr.opt.names)}, bufs={n: b.clone() for n, b in model.named_buffers()})
    head = [f"head.{br}_branch.3.{k}" for br in ("heatmap", "offset", "variance") for k in ("weight", "bias")]
    assert all(n in res[True]["grads"] and bool(res[True]["grads"][n].abs().sum() > 0) for n in head)
    assert same(res[True]["flat"], res[False]["flat"]) and same(res[True]["loss"], res[False]["loss"])
    for n, b in res[False]["bufs"].items():
        assert same(res[True]["bufs"][n], b), n
    differ = [n for n, g in res[False]["grads"].items() if not same(res[True]["grads"][n], g)]
    assert not differ, differ
    assert same(res[True]["grad"], res[False]["grad"])
