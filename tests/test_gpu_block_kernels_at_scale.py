"""GPU tests (`-m gpu`) of the transformer-block kernels (csrc/pk_block_mlp.hip, csrc/pk_block_attn.hip, csrc/pk_attn.hip, the weight-gradient and slab-reduction
kernels of csrc/pk_wgrad.hip) at the window and row counts training runs.

The block kernels are persistent: the release build caps every grid at a compile-time constant and each wave (or workgroup) walks
several windows / 32-row groups in a grid-stride loop, carrying register accumulators and LDS from one item to the next.  Only a
large tensor reaches the second and later iterations, so every case here is sized from the library's own size queries
(tests/test_host_cpu.py::test_block_kernel_cases_reach_their_loop_regimes checks that each one lands where its id says).
Entries are called through the C-ABI directly, so the partial buffers can be read.

Method, per case:
  1. the same entry runs once on the whole batch and once per sample (or per 512 windows): chunks small enough that every wave
     gets at most one item.  A window's / row's arithmetic does not depend on the wave or the iteration that computes it, so every
     per-token output must be BIT-EXACT between the two; a mismatch reports the items and the loop iterations
     (item // (waves x grid)) that produced it;
  2. reductions (LayerNorm dgamma / dbeta partials, rel-pos-bias partials, MLP weight slabs, weight and bias gradients) of the full
     launch against the float64 sum of the per-chunk results: both are fp32 sums of the SAME fp32 terms in another order, so they
     differ by at most L * U * 1.25 sum|term| (U = 2^-24; L = the two serial chain lengths, restated from the launch shapes;
     sum|term| from the float64 reference's own intermediates, x 1.25 for the distance between the kernel's terms and the
     reference's), and by at most 1e-4 of max|value| overall (a dropped window moves them by ~1e-2);
  3. a float64 reference at the full shape (rounding-aware as the older block tests: LayerNorm output rounded to bf16 where the
     kernel rounds it), error max|a - b| / max|b| taken PER SAMPLE and maximised over the samples, against the older tests' bars.
Inputs are bf16-representable, every channel has its own scale and offset, the rel-pos-bias table is random, and every sample has
its own DropPath scale (0 for b % 7 == 4, else (1 + b / 128) / 0.9), so a wrong sample index changes the result.  Outputs and
partial buffers start as NaN; dropped samples must give y == x and dx == dy bit for bit and contribute exact zeros.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
NAN = float("nan")
EPS = 1e-5
WS, AT_N = 7, 49


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def N():
    from infantposeestimation_gaussianbias_amd import nnops
    return nnops


def call(L, name, *args):
    L.call(name, *args, L.stream_ptr())


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def q(t):
    return t.to(BF).to(t.dtype)


def chan_data(rows, C, seed, offset=3.0, spread=0.5):
    """bf16 [rows][C]: channel c ~ N(off_c, s_c^2), s_c = 10^U(-spread, spread), |off_c| <= offset * s_c"""
    g = gen(seed)
    s = 10.0 ** ((torch.rand(C, generator=g, device=DEV, dtype=F64) * 2 - 1) * spread)
    off = (torch.rand(C, generator=g, device=DEV, dtype=F64) * 2 - 1) * offset * s
    return (torch.randn(rows, C, generator=g, device=DEV, dtype=F32).double() * s + off).to(BF)


def weight(n, k, seed, gain=1.0):
    """bf16 [n][k], row scale gain * 10^U(-0.3, 0.3) / sqrt(k)"""
    g = gen(seed)
    rs = gain * 10.0 ** ((torch.rand(n, 1, generator=g, device=DEV) * 2 - 1) * 0.3) / math.sqrt(k)
    return (torch.randn(n, k, generator=g, device=DEV) * rs).to(BF)


def vec(n, seed, base=0.0, spread=0.2):
    g = gen(seed)
    return q(base + spread * torch.randn(n, generator=g, device=DEV))


def drop_scales(B):
    """per-sample DropPath multiplier: 0 for b % 7 == 4, else (1 + b / 128) / 0.9 (fp32, as the kernels read it).  Samples 0 and 14 keep
    a non-zero scale: they hold the first and the second iteration's windows of the 1 050-window case."""
    b = torch.arange(B, dtype=F64)
    return torch.where(b % 7 == 4, torch.zeros_like(b), (1 + b / 128) / 0.9).float().to(DEV)


def nan_t(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(full, chunked, item_of_row, per_iter, what):
    """bit-exact equality of a per-token output; on failure: the differing items and their loop iterations"""
    assert full.shape == chunked.shape, what
    if torch.equal(bits(full), bits(chunked)):
        return
    rows = (bits(full) != bits(chunked)).reshape(full.shape[0], -1).any(1).nonzero().flatten()
    items = torch.unique(item_of_row[rows])
    items = items[items >= 0]
    it = torch.unique(items // per_iter)
    raise AssertionError(f"{what}: {rows.numel()} rows differ from the chunked launch; items {items[:12].tolist()} "
                         f"({items.numel()} in all), loop iterations {it.tolist()} (item // {per_iter})")


def order_only(full, chunked, abs_terms, chain, what):
    """two fp32 reductions of the same terms in another order: per element <= chain * U * 1.25 sum|term|, overall <= 1e-4 of max"""
    assert not torch.isnan(full).any() and not torch.isnan(chunked).any(), f"{what}: NaN left in the partials"
    d = (full.double() - chunked.double()).abs()
    bound = chain * U * 1.25 * abs_terms + 1e-30
    ratio = float((d / bound).max())
    rl = float(d.max() / chunked.double().abs().max().clamp_min(1e-30))
    print(f"{what}: order-only max|diff|/max = {rl:.3g}, worst diff / bound = {ratio:.3g}")
    if ratio > 1:
        i = int((d / bound).reshape(-1).argmax())
        raise AssertionError(f"{what}: outside the order-only bound at flat index {i}: full {float(full.reshape(-1)[i])!r}, chunked "
                             f"{float(chunked.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i])!r} (worst / bound {ratio:.3g})")
    assert rl <= 1e-4, f"{what}: max|diff| / max = {rl:.3g} > 1e-4"


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def per_sample(a, b, B, what, bar):
    """max over samples of max|a_s - b_s| / max|b_s|"""
    a, b = a.reshape(B, -1).double(), b.reshape(B, -1).double()
    e = (a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-30)
    worst = int(e.argmax())
    print(f"{what}: worst per-sample error {float(e[worst]):.3g} (sample {worst}), bar {bar}")
    assert float(e[worst]) < bar, f"{what}: sample {worst} error {float(e[worst]):.3g} >= {bar}"


def layer_norm64(x, gamma, beta, c_real=None):
    """float64 LayerNorm over the first c_real channels (the rest -> 0); returns (u, xhat)"""
    C = x.shape[-1]
    cr = c_real or C
    xr = x[..., :cr]
    mean = xr.mean(-1, keepdim=True)
    xhat = (xr - mean) / torch.sqrt(((xr - mean) ** 2).mean(-1, keepdim=True) + EPS)
    u = xhat * gamma[:cr] + beta[:cr]
    if cr < C:
        u = torch.cat([u, u.new_zeros(*u.shape[:-1], C - cr)], -1)
        xhat = torch.cat([xhat, xhat.new_zeros(*xhat.shape[:-1], C - cr)], -1)
    return u, xhat


def st_round(t):
    """rounded to bf16 in the forward, identity in the backward"""
    return t + (q(t) - t).detach()


_REL_IDX = {}


def rel_index():
    """[49 * 49] table row of every (query, key) pair, as oracle/nets.py rel_bias"""
    if "i" not in _REL_IDX:
        ys, xs = torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        _REL_IDX["i"] = ((ys[:, None] - ys[None, :] + WS - 1) * (2 * WS - 1) + (xs[:, None] - xs[None, :] + WS - 1)).reshape(-1).to(DEV)
    return _REL_IDX["i"]


def fold_table(pairs):
    """[Bw][heads][49][49] per-pair values -> [heads][169] table sums"""
    h = pairs.shape[1]
    return torch.zeros(169, h, dtype=pairs.dtype, device=DEV).index_add_(0, rel_index(), pairs.sum(0).permute(1, 2, 0).reshape(-1, h)).t()


def attn64(tok, wqkv, bqkv, table, wproj, bproj, heads, d=None, scale=None):
    """float64 window attention on (Bw, 49, C) tokens as oracle/nets.py window_attention (qkv, q * d^-0.5, QK^T + rel-pos bias,
    softmax, AV, proj; pad tokens attend), the head width `d` and the scale given for the padded twins; -> (out, logits)"""
    Bw, n, C = tok.shape
    d = d or C // heads
    qkv = (tok @ wqkv.T + bqkv).reshape(Bw, n, 3, heads, d)
    qq, kk, vv = qkv[:, :, 0] * (scale or d ** -0.5), qkv[:, :, 1], qkv[:, :, 2]
    bias = table[rel_index()].reshape(n, n, heads).permute(2, 0, 1)
    logits = torch.einsum("bnhd,bmhd->bhnm", qq, kk) + bias[None]
    o = torch.einsum("bhnm,bmhd->bnhd", torch.softmax(logits, -1), vv).reshape(Bw, n, heads * d)
    return o @ wproj.T + bproj, logits


def test_attention_reference_is_the_oracle():
    """attn64 restates oracle/nets.py window_attention (the large references below need its logits)"""
    from oracle import nets as onet
    C, heads = 64, 2
    tok = chan_data(6 * AT_N, C, 1).double().reshape(6, AT_N, C)
    P = {"a.qkv.weight": weight(3 * C, C, 2).double(), "a.qkv.bias": vec(3 * C, 3).double(), "a.proj.weight": weight(C, C, 4).double(),
         "a.proj.bias": vec(C, 5).double(), "a.relative_position_bias_table": vec(169 * heads, 6, spread=0.5).double().reshape(169, heads)}
    ref = onet.window_attention(tok.cpu(), {k: v.cpu() for k, v in P.items()}, "a", heads)
    got, _ = attn64(tok, P["a.qkv.weight"], P["a.qkv.bias"], P["a.relative_position_bias_table"], P["a.proj.weight"], P["a.proj.bias"], heads)
    assert torch.allclose(got.cpu(), ref, rtol=1e-12, atol=1e-12)


def win_of_row(rowmap, M):
    """pixel row -> window index (every pixel sits in exactly one window)"""
    w = torch.full((M,), -1, dtype=torch.int64, device=DEV)
    ok = rowmap >= 0
    w[rowmap[ok].long()] = (torch.arange(rowmap.numel(), device=DEV) // AT_N)[ok]
    return w


# ================================================================================================ fused attention half
class AttnCase:
    def __init__(self, N, Cc, heads, B, H, W, seed):
        self.C, self.heads, self.B, self.H, self.W = Cc, heads, B, H, W
        self.M, self.HW = B * H * W, H * W
        self.x = chan_data(self.M, Cc, seed)
        self.dy = chan_data(self.M, Cc, seed + 1, offset=0.3)
        self.gamma, self.beta = vec(Cc, seed + 2, 1.0, 0.3), vec(Cc, seed + 3)
        self.table = vec(169 * heads, seed + 4, spread=0.5).reshape(169, heads).contiguous()
        self.wqkv, self.bqkv = weight(3 * Cc, Cc, seed + 5, 2.0), vec(3 * Cc, seed + 6)
        self.wproj, self.bproj = weight(Cc, Cc, seed + 7), vec(Cc, seed + 8)
        self.wqkv_t, self.wproj_t = self.wqkv.t().contiguous(), self.wproj.t().contiguous()
        self.s = drop_scales(B)
        self.rowmap, self.nwin = N.window_rowmap(B, H, W, DEV)
        self.rowmap1, _ = N.window_rowmap(1, H, W, DEV)
        self.nw = B * self.nwin

    def fwd(self, L, b0, nb, save=True):
        HW, C = self.HW, self.C
        nw = nb * self.nwin
        rm = self.rowmap if nb == self.B else self.rowmap1
        y = nan_t((nb * HW, C), BF)
        o = nan_t((nw * AT_N, C), BF) if save else None
        lse = nan_t((nw * self.heads * AT_N,)) if save else None
        call(L, "pk_attn_block_fwd", self.x[b0 * HW:(b0 + nb) * HW], rm, self.gamma, self.beta, self.table, self.wqkv, self.bqkv, self.wproj,
             self.bproj, self.s[b0:b0 + nb], y, o, lse, nw, self.nwin, self.heads, C, EPS)
        return y, o, lse

    def bwd(self, L, b0, nb, o, lse):
        HW, C = self.HW, self.C
        nw = nb * self.nwin
        sl = slice(b0 * HW, (b0 + nb) * HW)
        rm = self.rowmap if nb == self.B else self.rowmap1
        blocks = L.lib.pk_attn_block_blocks(nw)
        r = dict(dx=nan_t((nb * HW, C), BF), dqkv=nan_t((nw * AT_N, 3 * C), BF), u=nan_t((nw * AT_N, C), BF),
                 ln=nan_t((blocks, 2, C)), rpb=nan_t((blocks * 4, self.heads, 169)))
        call(L, "pk_attn_block_bwd", self.dy[sl], self.x[sl], rm, self.gamma, self.beta, self.table, self.wqkv, self.bqkv, self.wqkv_t,
             self.wproj_t, self.s[b0:b0 + nb], o, lse, r["dx"], r["dqkv"], r["u"], r["ln"], r["rpb"], nw, self.nwin, self.heads, C, EPS)
        return r

    def reference(self):
        """float64 forward (LayerNorm output rounded to bf16, the kernel's MFMA operand) and autograd backward (unrounded, as the older
        backward test), plus the |terms| of the reductions"""
        from oracle import nets as onet
        B, H, W, C, heads = self.B, self.H, self.W, self.C, self.heads
        x = self.x.double().reshape(B, H, W, C).requires_grad_(True)
        P = [t.double().requires_grad_(True) for t in (self.gamma, self.beta, self.table, self.wqkv, self.bqkv, self.wproj, self.bproj)]
        g1, b1, tab, wq, bq, wp, bp = P
        s = self.s.double().view(B, 1, 1, 1)
        with torch.no_grad():
            u, _ = layer_norm64(x, g1, b1)
            tok, (Hp, Wp) = onet.to_windows(q(u))
            y_ref = (x + onet.from_windows(attn64(tok, wq, bq, tab, wp, bp, heads)[0], B, H, W, Hp, Wp) * s).reshape(self.M, C)
        u, xhat = layer_norm64(x, g1, b1)
        u.retain_grad()
        tok, (Hp, Wp) = onet.to_windows(u)
        a, logits = attn64(tok, wq, bq, tab, wp, bp, heads)
        logits.retain_grad()
        (x + onet.from_windows(a, B, H, W, Hp, Wp) * s).backward(self.dy.double().reshape(B, H, W, C))
        du, xh = u.grad.reshape(self.M, C), xhat.detach().reshape(self.M, C)
        return dict(y=y_ref, dx=x.grad.reshape(self.M, C), grads=[p.grad for p in P], ln_abs=((du * xh).abs().sum(0), du.abs().sum(0)),
                    tab_abs=fold_table(logits.grad.abs()))


ATTN_CASES = [
    # C, heads, B, H, W -- HRFormer-small branch 0 at B = 64: 4 480 windows on 1 024 waves, 4.4 windows per wave
    pytest.param(32, 1, 64, 64, 48, id="C32-B64-4480win-4.4perwave"),
    # 1 050 windows: 26 waves take a second window
    pytest.param(32, 1, 15, 64, 48, id="C32-B15-1050win-26waves-second"),
    # branch 1 at B = 64: 1 280 windows, 1.25 per wave (ragged)
    pytest.param(64, 2, 64, 32, 24, id="C64-B64-1280win-ragged"),
]


@pytest.mark.parametrize("Cc,heads,B,H,W", ATTN_CASES)
def test_fused_attention_half_at_training_window_counts(L, N, Cc, heads, B, H, W):
    """pk_attn_block_fwd (save on and off) and pk_attn_block_bwd at several windows per wave (k_attn_bwd carries its per-wave LDS
    rel-pos-bias gradient sTab and the LayerNorm sums across windows): against per-sample launches (one window per wave) bit for bit,
    the dgamma / dbeta / rel-pos-bias partials order-only, and a float64 reference per sample."""
    cs = AttnCase(N, Cc, heads, B, H, W, seed=Cc + B)
    HW, nwin = cs.HW, cs.nwin
    blocks = L.lib.pk_attn_block_blocks(cs.nw)
    per_iter = 4 * blocks
    assert cs.nw > per_iter, "the full launch must give some wave a second window"
    y, o, lse = cs.fwd(L, 0, B, save=True)
    y2, _, _ = cs.fwd(L, 0, B, save=False)
    r = cs.bwd(L, 0, B, o, lse)
    bc = L.lib.pk_attn_block_blocks(nwin)
    assert nwin <= 4 * bc, "a per-sample launch must give every wave at most one window"
    parts = []
    for b in range(B):
        yc, oc, lc = cs.fwd(L, b, 1)
        parts.append((yc, oc, lc, cs.bwd(L, b, 1, oc, lc)))
    torch.cuda.synchronize()
    wrow = win_of_row(cs.rowmap, cs.M)
    wtok = torch.arange(cs.nw * AT_N, device=DEV) // AT_N
    same(y2, y, wrow, per_iter, "y with save off vs save on")
    same(y, torch.cat([p[0] for p in parts]), wrow, per_iter, "y")
    same(o, torch.cat([p[1] for p in parts]), wtok, per_iter, "o")
    same(lse.reshape(cs.nw, -1), torch.cat([p[2] for p in parts]).reshape(cs.nw, -1), torch.arange(cs.nw, device=DEV), per_iter, "lse")
    for k in ("dx", "dqkv", "u"):
        same(r[k], torch.cat([p[3][k] for p in parts]), wrow if k == "dx" else wtok, per_iter, k)
    # dropped samples: the half is the identity and contributes exact zeros to every reduction
    for b in range(4, B, 7):
        sl = slice(b * HW, (b + 1) * HW)
        assert torch.equal(bits(y[sl]), bits(cs.x[sl])) and torch.equal(bits(r["dx"][sl]), bits(cs.dy[sl])), b
        assert torch.count_nonzero(parts[b][3]["ln"]) == 0 and torch.count_nonzero(parts[b][3]["rpb"]) == 0, b
    # nothing keeps a NaN; the waves of a per-sample launch that get no window write zero partials
    for rc in [r] + [p[3] for p in parts]:
        assert not torch.isnan(rc["ln"]).any() and not torch.isnan(rc["rpb"]).any()
    if 4 * bc > nwin:
        assert torch.count_nonzero(parts[1][3]["rpb"][nwin:]) == 0
    # order-only: the full launch's reductions vs the float64 sum of the per-sample launches'
    ref = cs.reference()
    tag = f"attn C={Cc} B={B}"
    ln_full = r["ln"].double().sum(0)
    ln_chunk = sum(p[3]["ln"].double().sum(0) for p in parts)
    chain_ln = (-(-cs.nw // blocks) + -(-nwin // bc)) * AT_N + 16
    order_only(ln_full[0], ln_chunk[0], ref["ln_abs"][0], chain_ln, f"{tag} dgamma partials")
    order_only(ln_full[1], ln_chunk[1], ref["ln_abs"][1], chain_ln, f"{tag} dbeta partials")
    rp_full = r["rpb"].double().sum(0)
    rp_chunk = sum(p[3]["rpb"].double().sum(0) for p in parts)
    order_only(rp_full, rp_chunk, ref["tab_abs"], (-(-cs.nw // per_iter) + 1) * AT_N + 64, f"{tag} rel-pos-bias partials")
    # float64 reference at the full shape, per sample
    per_sample(y, ref["y"], B, f"{tag} y", 1.5e-2)
    per_sample(r["dx"], ref["dx"], B, f"{tag} dx", 3e-2)
    g = ref["grads"]
    for name, got, gr in (("dgamma", ln_full[0], g[0]), ("dbeta", ln_full[1], g[1]), ("dtable", rp_full, g[2].t())):
        e = rel(got, gr)
        print(f"{tag} {name} vs float64: {e:.3g}")
        assert e < 3e-2, (name, e)


# ================================================================================================ fused MLP half
class MlpCase:
    def __init__(self, Cc, B, H, W, seed):
        self.C, self.B, self.H, self.W = Cc, B, H, W
        self.M, self.HW, self.Hd = B * H * W, H * W, 4 * Cc
        self.x = chan_data(self.M, Cc, seed)
        self.dy = chan_data(self.M, Cc, seed + 1, offset=0.3)
        self.gamma, self.beta = vec(Cc, seed + 2, 1.0, 0.3), vec(Cc, seed + 3)
        self.w1, self.b1 = weight(self.Hd, Cc, seed + 4, 2.0), vec(self.Hd, seed + 5)
        self.w2, self.b2 = weight(Cc, self.Hd, seed + 6), vec(Cc, seed + 7)
        self.w1_t, self.w2_t = self.w1.t().contiguous(), self.w2.t().contiguous()
        self.s = drop_scales(B)

    def run(self, L, b0, nb):
        C, HW = self.C, self.HW
        M = nb * HW
        sl = slice(b0 * HW, (b0 + nb) * HW)
        nbx, nbw = L.lib.pk_ln_mlp_dx_blocks(M, C), L.lib.pk_ln_mlp_dw_blocks(M, C)
        HS, SL = L.lib.pk_ln_mlp_hidden_slice(C), L.lib.pk_ln_mlp_slab_floats(C)
        r = dict(y=nan_t((M, C), BF), dx=nan_t((M, C), BF), ln=nan_t((nbx, 2, C)), slabs=nan_t((self.Hd // HS, nbw, SL)), nbx=nbx, nbw=nbw)
        s = self.s[b0:b0 + nb]
        call(L, "pk_ln_mlp_fwd", self.x[sl], self.gamma, self.beta, self.w1, self.b1, self.w2, self.b2, s, r["y"], M, C, HW, EPS)
        call(L, "pk_ln_mlp_bwd_dx", self.dy[sl], self.x[sl], self.gamma, self.beta, self.w1, self.b1, self.w1_t, self.w2_t, s, r["dx"],
             r["ln"], M, C, HW, EPS)
        call(L, "pk_ln_mlp_bwd_dw", self.dy[sl], self.x[sl], self.gamma, self.beta, self.w1, self.b1, self.w2_t, s, r["slabs"], M, C, HW, EPS)
        return r

    def unpack(self, L, slabs):
        """slabs [slices][blocks][SL] summed over the blocks in float64 -> dW1 [4C][C], dW2 [C][4C], db1 [4C], db2 of every slice"""
        C, HS = self.C, L.lib.pk_ln_mlp_hidden_slice(self.C)
        t = slabs.double().sum(1)
        ns = t.shape[0]
        dw1 = t[:, :HS * C].reshape(ns * HS, C)
        dw2 = t[:, HS * C:2 * HS * C].reshape(ns, C, HS).permute(1, 0, 2).reshape(C, ns * HS)
        return dw1, dw2, t[:, 2 * HS * C:2 * HS * C + HS].reshape(-1), t[:, 2 * HS * C + HS:]

    def reference(self):
        x = self.x.double().requires_grad_(True)
        P = [t.double().requires_grad_(True) for t in (self.gamma, self.beta, self.w1, self.b1, self.w2, self.b2)]
        g2, bt2, w1, b1, w2, b2 = P
        srow = self.s.repeat_interleave(self.HW)[:, None]
        v, xhat = layer_norm64(x, g2, bt2)
        v.retain_grad()
        vq = st_round(v)
        z = vq @ w1.T + b1
        h = F.gelu(z)
        y = x + (h @ w2.T + b2) * srow.double()
        y.backward(self.dy.double())
        with torch.no_grad():
            gs = q(self.dy.float() * srow).double()                 # the kernel's bf16 (s * dy) operand
            dz = (gs @ w2) * (0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
            dv = v.grad
            ab = dict(dgamma=(dv * xhat).abs().sum(0), dbeta=dv.abs().sum(0), dw1=dz.abs().T @ vq.abs(), dw2=gs.abs().T @ h.abs(),
                      db1=dz.abs().sum(0), db2=gs.abs().sum(0))
        return dict(y=y.detach(), dx=x.grad, grads=[p.grad for p in P], abs=ab)


def rows_per_wave(M, blocks):
    """rows of the longest walk of a 4-wave-per-workgroup launch over 32-row groups"""
    return 32 * -(-(-(-M // 32)) // (4 * blocks))


MLP_CASES = [
    # C, B, H, W -- HRFormer-small branch 0 at B = 64: M = 196 608, 3 row groups per wave in fwd / dx, 6 in dw
    pytest.param(32, 64, 64, 48, id="C32-M196608-dw6perwave"),
    # branch 1 at B = 64: M = 49 152, 32 dw workgroups x 8 slices, 12 row groups per wave
    pytest.param(64, 64, 32, 24, id="C64-M49152-dw12perwave"),
    # ragged: M = 62 403 (M % 32 = 3), samples of 1 023 rows straddle the 32-row groups
    pytest.param(64, 61, 33, 31, id="C64-M62403-ragged"),
]


@pytest.mark.parametrize("Cc,B,H,W", MLP_CASES)
def test_fused_mlp_half_at_training_row_counts(L, Cc, B, H, W):
    """pk_ln_mlp_fwd / _bwd_dx / _bwd_dw at several 32-row groups per wave (k_mlp_bwd_dw carries its weight-gradient accumulators over
    the whole walk): against per-sample launches (one group per wave) bit for bit, the LayerNorm partials and the weight / bias slabs
    order-only, and a float64 reference per sample."""
    cs = MlpCase(Cc, B, H, W, seed=Cc + B + 100)
    M, HW = cs.M, cs.HW
    r = cs.run(L, 0, B)
    assert -(-M // 32) > 4 * r["nbw"], "the full dw launch must give some wave a second row group"
    parts = [cs.run(L, b, 1) for b in range(B)]
    assert -(-HW // 32) <= 4 * min(parts[0]["nbx"], parts[0]["nbw"])
    torch.cuda.synchronize()
    grp = torch.arange(M, device=DEV) // 32
    same(r["y"], torch.cat([p["y"] for p in parts]), grp, 4 * L.lib.pk_ln_mlp_dx_blocks(M, Cc), "y")
    same(r["dx"], torch.cat([p["dx"] for p in parts]), grp, 4 * r["nbx"], "dx")
    for b in range(4, B, 7):
        sl = slice(b * HW, (b + 1) * HW)
        assert torch.equal(bits(r["y"][sl]), bits(cs.x[sl])) and torch.equal(bits(r["dx"][sl]), bits(cs.dy[sl])), b
        assert torch.count_nonzero(parts[b]["ln"]) == 0 and torch.count_nonzero(parts[b]["slabs"]) == 0, b
    for rc in [r] + parts:
        assert not torch.isnan(rc["ln"]).any() and not torch.isnan(rc["slabs"]).any()
    ref = cs.reference()
    ab, tag = ref["abs"], f"mlp C={Cc} M={M}"
    chain_dx = rows_per_wave(M, r["nbx"]) + rows_per_wave(HW, parts[0]["nbx"]) + 64
    chain_dw = rows_per_wave(M, r["nbw"]) + rows_per_wave(HW, parts[0]["nbw"]) + 64
    ln_full, ln_chunk = r["ln"].double().sum(0), sum(p["ln"].double().sum(0) for p in parts)
    order_only(ln_full[0], ln_chunk[0], ab["dgamma"], chain_dx, f"{tag} dgamma partials")
    order_only(ln_full[1], ln_chunk[1], ab["dbeta"], chain_dx, f"{tag} dbeta partials")
    full = cs.unpack(L, r["slabs"])
    chunk = [sum(t) for t in zip(*(cs.unpack(L, p["slabs"]) for p in parts))]
    for name, f_, c_ in zip(("dW1", "dW2", "db1"), full[:3], chunk[:3]):
        order_only(f_, c_, ab[name.lower()], chain_dw, f"{tag} {name} slabs")
    for y_ in range(full[3].shape[0]):                  # db2 is complete in every hidden slice
        order_only(full[3][y_], chunk[3][y_], ab["db2"], chain_dw, f"{tag} db2 slabs (slice {y_})")
    per_sample(r["y"], ref["y"], B, f"{tag} y", 8e-3)
    per_sample(r["dx"], ref["dx"], B, f"{tag} dx", 1e-2)
    g = ref["grads"]
    for name, got, gr in (("dgamma", ln_full[0], g[0]), ("dbeta", ln_full[1], g[1]), ("dW1", full[0], g[2]), ("db1", full[2], g[3]),
                          ("dW2", full[1], g[4]), ("db2", full[3][0], g[5])):
        e = rel(got, gr)
        print(f"{tag} {name} vs float64: {e:.3g}")
        assert e < 1e-2, (name, e)


# ================================================================================================ unfused window attention (branch 1)
WATTN_CASES = [
    # d, heads, windows -- d = 32 with 2 heads at 1 280 windows: 2 windows per workgroup
    pytest.param(32, 2, 1280, id="d32-h2-1280win-2pergroup"),
    # d = 32, 1 head, 4 480 windows: 3 windows per workgroup, 1 494 groups per head (> 256: several passes of k_relbias_reduce)
    pytest.param(32, 1, 4480, id="d32-h1-4480win-3pergroup"),
    # d = 40 (the padded head of the HRFormer-base twin), 2 heads, 4 480 windows: 5 windows per workgroup, 896 groups per head
    pytest.param(40, 2, 4480, id="d40-h2-4480win-5pergroup"),
]


@pytest.mark.parametrize("d,heads,nw", WATTN_CASES)
def test_window_attention_at_training_window_counts(L, N, d, heads, nw):
    """pk_window_attn_fwd / _bwd (branch 1's training path) with several windows per workgroup (k_win_attn_bwd keeps the bias
    gradient in registers across them); the table gradient reduced by k_relbias_reduce (dtable given) and, as production does, from
    the partials by pk_reduce_many (dtable NULL).  Against launches of 512 windows (one window per workgroup) bit for bit, the partials
    order-only, both reductions against the float64 sum of the partials and each other, and a float64 reference per 64 windows."""
    C = heads * d
    seed = 300 + d + heads
    qkv = chan_data(nw * AT_N, 3 * C, seed, offset=0.5)
    dout = chan_data(nw * AT_N, C, seed + 1, offset=0.2)
    table = vec(169 * heads, seed + 2, spread=0.5).reshape(169, heads).contiguous()
    per_head = L.lib.pk_window_attn_bwd_groups(nw, heads) // heads
    assert nw > per_head

    def run(w0, n, with_table):
        o, lse = nan_t((n * AT_N, C), BF), nan_t((n * heads * AT_N,))
        sl = slice(w0 * AT_N, (w0 + n) * AT_N)
        call(L, "pk_window_attn_fwd", qkv[sl], table, o, lse, n, heads, C, 0.0)
        dq = nan_t((n * AT_N, 3 * C), BF)
        part = nan_t((L.lib.pk_window_attn_bwd_ws_floats(n, heads),))
        dt = nan_t((169, heads)) if with_table else None
        call(L, "pk_window_attn_bwd", qkv[sl], table, o, dout[sl], lse, dq, part, dt, n, heads, C, 0.0)
        return o, lse, dq, part.reshape(-1, heads, 169), dt

    o, lse, dq, part, dt = run(0, nw, True)
    _, _, dq0, part0, _ = run(0, nw, False)
    dt_many = nan_t((169 + 8, heads))                  # 8 guard rows: no write past K
    N._reduce([N._row(part=(part0, 169 * hh), out=(dt_many, hh), stride=169 * heads, S=per_head, K=169, ostride=heads)
               for hh in range(heads)], False, torch.device(DEV))
    chunks = []
    for w0 in range(0, nw, 512):
        n = min(512, nw - w0)
        assert L.lib.pk_window_attn_bwd_groups(n, heads) == n * heads       # one window per workgroup
        chunks.append(run(w0, n, True))
    torch.cuda.synchronize()
    wt = torch.arange(nw * AT_N, device=DEV) // AT_N
    same(o, torch.cat([c[0] for c in chunks]), wt, nw, "o")
    same(lse.reshape(nw, -1), torch.cat([c[1] for c in chunks]).reshape(nw, -1), torch.arange(nw, device=DEV), nw, "lse")
    same(dq, torch.cat([c[2] for c in chunks]), wt, per_head, "dqkv")
    same(dq0, dq, wt, per_head, "dqkv of the NULL-table launch")
    assert torch.equal(bits(part0), bits(part)), "the partials do not depend on the table path"
    assert not torch.isnan(part).any() and not torch.isnan(dt).any()
    assert torch.isnan(dt_many[169:]).all(), "pk_reduce_many wrote past K"
    dt_many = dt_many[:169]
    # partials [groups][169], group g = k * heads + h belongs to head h
    p64 = part.double().reshape(per_head, heads, 169)
    full64 = p64.sum(0)
    chunk64 = sum(c[3].double().reshape(-1, heads, 169).sum(0) for c in chunks)
    qk = qkv.double().requires_grad_(True)
    t5 = qk.reshape(nw, AT_N, 3, heads, d)
    bias = table.double()[rel_index()].reshape(AT_N, AT_N, heads).permute(2, 0, 1)
    logits = torch.einsum("bnhd,bmhd->bhnm", t5[:, :, 0] * d ** -0.5, t5[:, :, 1]) + bias[None]
    logits.retain_grad()
    o_ref = torch.einsum("bhnm,bmhd->bnhd", torch.softmax(logits, -1), t5[:, :, 2]).reshape(nw * AT_N, C)
    o_ref.backward(dout.double())
    tag = f"window attn d={d} heads={heads} windows={nw}"
    order_only(full64, chunk64, fold_table(logits.grad.abs()), (-(-nw // per_head) + 1) * AT_N + 64, f"{tag} rel-pos-bias partials")
    # the two fp32 reductions of the SAME partials (terms = the partials): each vs their float64 sum, and each other
    pabs = p64.abs().sum(0)
    c_rb, c_rm = -(-per_head // 256) + 8, -(-per_head // 16) + 16
    for name, got, chain in (("k_relbias_reduce", dt, c_rb), ("pk_reduce_many", dt_many, c_rm)):
        ratio = float(((got.double().t() - full64).abs() / (chain * U * pabs + 1e-30)).max())
        print(f"{tag} dtable by {name} vs float64 of the partials: worst / bound {ratio:.3g}")
        assert ratio <= 1, (name, ratio)
    order_only(dt, dt_many, pabs.t() / 1.25, c_rb + c_rm, f"{tag} dtable: k_relbias_reduce vs pk_reduce_many")
    per_sample(o, o_ref.detach(), nw // 64, f"{tag} o", 1.5e-2)
    per_sample(dq, qk.grad, nw // 64, f"{tag} dqkv", 3e-2)
    e = rel(dt.t(), fold_table(logits.grad))
    print(f"{tag} dtable vs float64: {e:.3g}")
    assert e < 3e-2


# ================================================================================================ wide forward kernels (cfg 5 sizes)
def test_wide_fused_attention_forward_at_cfg5_windows(L, N):
    """pk_attn_block_wide_fwd, C = 80 with 2 heads of the padded head_dim 39 (HRFormer-base twin, branch 0 of cfg 5: B = 128, 64 x 48,
    8 960 windows on 256 workgroups x 8 waves = 4.4 windows per wave): against per-sample launches (70 windows, one per wave) bit for
    bit and against the float64 oracle half of the real 78-channel block per sample; the padded output channels stay 0."""
    from oracle import nets as onet
    B, H, W, heads, d, dp, Cc = 128, 64, 48, 2, 39, 40, 80
    Cr, HW, M = heads * d, H * W, B * H * W
    xr = chan_data(M, Cr, 500)
    g1, b1 = vec(Cr, 501, 1.0, 0.3), vec(Cr, 502)
    table = vec(169 * heads, 503, spread=0.5).reshape(169, heads).contiguous()
    wq, bq, wp, bp = weight(3 * Cr, Cr, 504, 2.0), vec(3 * Cr, 505), weight(Cr, Cr, 506), vec(Cr, 507)
    s = drop_scales(B)
    # the twin, embedded as models/padded.py does: plain tensors zero-extended, the head dimension padded per head
    hsel = torch.cat([torch.arange(d) + dp * h for h in range(heads)]).to(DEV)
    rows3 = torch.cat([hsel + part * Cc for part in range(3)])
    ar = torch.arange(Cr, device=DEV)
    x = torch.zeros(M, Cc, dtype=BF, device=DEV)
    x[:, :Cr] = xr
    tg1, tb1, tbq, tbp = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.zeros(3 * Cc, device=DEV), torch.zeros(Cc, device=DEV)
    tg1[:Cr], tb1[:Cr], tbq[rows3], tbp[:Cr] = g1, b1, bq, bp
    twq, twp = torch.zeros(3 * Cc, Cc, dtype=BF, device=DEV), torch.zeros(Cc, Cc, dtype=BF, device=DEV)
    twq[rows3.unsqueeze(1), ar] = wq
    twp[ar.unsqueeze(1), hsel] = wp
    rowmap, nwin = N.window_rowmap(B, H, W, DEV)
    rowmap1, _ = N.window_rowmap(1, H, W, DEV)
    assert B * nwin > 256 * 8 and nwin <= 8 * -(-nwin // 8)

    def run(b0, nb):
        y = nan_t((nb * HW, Cc), BF)
        call(L, "pk_attn_block_wide_fwd", x[b0 * HW:(b0 + nb) * HW], rowmap if nb == B else rowmap1, tg1, tb1, table, twq, tbq, twp, tbp,
             s[b0:b0 + nb], y, nb * nwin, nwin, heads, Cc, Cr, d ** -0.5, EPS)
        return y

    y = run(0, B)
    yc = torch.cat([run(b, 1) for b in range(B)])
    torch.cuda.synchronize()
    same(y, yc, win_of_row(rowmap, M), 256 * 8, "wide attention y")
    assert torch.count_nonzero(y[:, Cr:]) == 0
    for b in range(4, B, 7):
        assert torch.equal(bits(y[b * HW:(b + 1) * HW]), bits(x[b * HW:(b + 1) * HW])), b
    with torch.no_grad():
        x64 = xr.double().reshape(B, H, W, Cr)
        u, _ = layer_norm64(x64, g1.double(), b1.double())
        tok, (Hp, Wp) = onet.to_windows(q(u))
        a, _ = attn64(tok, wq.double(), bq.double(), table.double(), wp.double(), bp.double(), heads)
        y_ref = x64 + onet.from_windows(a, B, H, W, Hp, Wp) * s.double().view(B, 1, 1, 1)
    per_sample(y[:, :Cr], y_ref, B, "wide attention y", 1.5e-2)


@pytest.mark.parametrize("Cc,hidden,B,H,W", [
    # C = 80, hidden 320 (the only production width whose weights fit the resident path): 393 216 rows = 1 536 tiles of 256 rows on
    # one workgroup per CU, ~6 tiles per workgroup
    pytest.param(80, 320, 128, 64, 48, id="C80-h320-M393216-resident-6tiles"),
    # C = 160, hidden 640 (weights streamed through LDS, one workgroup per tile) at 98 304 rows
    pytest.param(160, 640, 128, 32, 24, id="C160-h640-M98304-streamed"),
])
def test_wide_fused_mlp_forward_at_cfg5_rows(L, Cc, hidden, B, H, W):
    """pk_ln_mlp_wide_fwd at cfg 5 row counts: against per-sample launches (a handful of 256-row tiles, one per workgroup) bit for bit
    and against a float64 reference per sample; dropped samples give y == x."""
    M, HW = B * H * W, H * W
    x = chan_data(M, Cc, 600 + Cc)
    g2, b2 = vec(Cc, 601, 1.0, 0.3), vec(Cc, 602)
    w1, bb1, w2, bb2 = weight(hidden, Cc, 603, 2.0), vec(hidden, 604), weight(Cc, hidden, 605), vec(Cc, 606)
    s = drop_scales(B)
    assert L.lib.pk_ln_mlp_wide_supported(Cc, hidden, M)

    def run(b0, nb):
        y = nan_t((nb * HW, Cc), BF)
        call(L, "pk_ln_mlp_wide_fwd", x[b0 * HW:(b0 + nb) * HW], g2, b2, w1, bb1, w2, bb2, s[b0:b0 + nb], y, nb * HW, Cc, Cc, hidden, HW, EPS)
        return y

    y = run(0, B)
    yc = torch.cat([run(b, 1) for b in range(B)])
    torch.cuda.synchronize()
    same(y, yc, torch.arange(M, device=DEV) // 256, 256, "wide mlp y")
    for b in range(4, B, 7):
        assert torch.equal(bits(y[b * HW:(b + 1) * HW]), bits(x[b * HW:(b + 1) * HW])), b
    worst = 0.0
    for b0 in range(0, B, 16):                       # float64 reference in pieces of 16 samples
        sl = slice(b0 * HW, (b0 + 16) * HW)
        with torch.no_grad():
            x64 = x[sl].double()
            v, _ = layer_norm64(x64, g2.double(), b2.double())
            m = F.gelu(q(v) @ w1.double().T + bb1.double()) @ w2.double().T + bb2.double()
            y_ref = x64 + m * s[b0:b0 + 16].double().repeat_interleave(HW)[:, None]
        a, r_ = y[sl].double().reshape(16, -1), y_ref.reshape(16, -1)
        worst = max(worst, float(((a - r_).abs().amax(1) / r_.abs().amax(1)).max()))
    print(f"wide mlp C={Cc}: worst per-sample error {worst:.3g}, bar 8e-3")
    assert worst < 8e-3


# ================================================================================================ block level: autograd functions
def _capture_wgrad(N, monkeypatch):
    """record every nnops._wgrad call (operands, maps, scale, destinations) of a backward pass"""
    calls = []
    real = N._wgrad

    def wrapped(x, g, Nn, Cin, ksize, stride, geom, a_map=None, g_map=None, g_scale=None, g_rps=0, M=None, oihw=True, out=None, dbias=None,
                deferred=False, win=None):
        res = real(x, g, Nn, Cin, ksize, stride, geom, a_map=a_map, g_map=g_map, g_scale=g_scale, g_rps=g_rps, M=M, oihw=oihw, out=out,
                   dbias=dbias, deferred=deferred, win=win)
        calls.append(dict(x=x, g=g, N=Nn, Cin=Cin, a_map=a_map, g_map=g_map, g_scale=g_scale, g_rps=g_rps, M=M, dw=res, dbias=dbias, win=win))
        return res

    monkeypatch.setattr(N, "_wgrad", wrapped)
    return calls


def _check_wgrad(L, c, what):
    """a weight / bias gradient against float64 G'^T X' of the kernel's own bf16 operands (rows gathered through the maps, -1 -> 0; G
    rows times the sample's scale, rounded to bf16 as the kernel does); per element (rows per slice + slices + 64) * U * sum|term|"""
    M = c["M"]
    flags = (1 if c["a_map"] is not None else 0) | (2 if c["g_map"] is not None else 0) | (4 if c["g_scale"] is not None else 0)
    _, Hs, Ws = c["win"] if c["win"] is not None else (0, 0, 0)
    S = L.lib.pk_wgrad_slices(M, c["N"], c["Cin"], 1, 1, Hs, Ws, flags)

    def gather(t, m):
        if m is None:
            return t[:M].float()
        return torch.where((m >= 0)[:, None], t[m.long().clamp_min(0)].float(), torch.zeros((), device=DEV))

    X = gather(c["x"].reshape(-1, c["Cin"]), c["a_map"]).double()
    G = gather(c["g"].reshape(-1, c["N"]), c["g_map"])
    if c["g_scale"] is not None:
        src = c["g_map"].long() if c["g_map"] is not None else torch.arange(M, device=DEV)
        G = q(G * c["g_scale"][src.clamp_min(0) // c["g_rps"]][:, None])
    G = G.double()
    chain = -(-M // S) + S + 64
    for name, got, ref, ab in (("dW", c["dw"], G.T @ X, G.abs().T @ X.abs()), ("dbias", c["dbias"], G.sum(0), G.abs().sum(0))):
        got = got.reshape(ref.shape).double()
        ratio = float(((got - ref).abs() / (chain * U * ab + 1e-30)).max())
        print(f"{what} {name} (M={M}, S={S}, flags={flags}): worst / bound {ratio:.3g}, max-norm {rel(got, ref):.3g}")
        assert ratio <= 1, (what, name, ratio)
    assert S >= 2, (what, M, S)
    return flags


BLOCK_CASES = [
    # half, C, heads, H, W at B = 64: the fused halves of branch 0, the unfused training paths of branches 1 (attention) and 2 (MLP)
    pytest.param("attn_fused", 32, 1, 64, 48, id="AttnHalfFused-C32"),
    pytest.param("mlp_fused", 32, 1, 64, 48, id="MlpHalfFused-C32"),
    pytest.param("attn", 64, 2, 32, 24, id="AttnHalf-C64"),
    pytest.param("mlp", 128, 4, 16, 12, id="MlpHalf-C128"),
]


@pytest.mark.parametrize("defer", ["0", "1"])
@pytest.mark.parametrize("half,Cc,heads,H,W", BLOCK_CASES)
def test_block_halves_at_batch_64(L, N, monkeypatch, half, Cc, heads, H, W, defer):
    """The autograd functions of nnops at B = 64 with gradient sinks (NaN-filled) and POSE_DEFER_REDUCE = 0 (slab reductions inside
    backward) or 1 (postponed to one pk_reduce_many): every weight / bias gradient of the four GEMMs against float64 G'^T X' of its own
    operands at production slice counts (plain k_wgrad4: fused qkv, fc1; k_wgrad4w mode 1: qkv with the window map, mode 2: proj with
    map and scale, mode 3: fc2 with scale), and y / dx per sample and every parameter gradient against a float64 autograd reference."""
    from infantposeestimation_gaussianbias_amd.models.hrformer import HRFormerBlock
    from oracle import nets as onet
    monkeypatch.setenv("POSE_DEFER_REDUCE", defer)
    B = 64
    M = B * H * W
    blk = HRFormerBlock(Cc, heads).to(DEV)
    with torch.no_grad():
        for i, (n, p) in enumerate(blk.named_parameters()):
            if p.dim() == 2:
                p.copy_(weight(p.shape[0], p.shape[1], 700 + i, 2.0 if ("qkv" in n or "fc1" in n) else 1.0).float())
            else:
                p.copy_(vec(p.numel(), 700 + i, 1.0 if n.startswith("norm") and n.endswith("weight") else 0.0))
    x = chan_data(M, Cc, 710 + Cc).reshape(B, H, W, Cc)
    dy = chan_data(M, Cc, 711 + Cc, offset=0.3).reshape(B, H, W, Cc)
    s = drop_scales(B)
    calls = _capture_wgrad(N, monkeypatch)
    N.begin_grad_epoch()
    for p in blk.parameters():
        p._pk_grad_sink = torch.full_like(p, NAN)
    a, m = blk.attn, blk.mlp
    xd = x.clone().requires_grad_(True)
    with N.use_weights(blk):
        if half in ("attn_fused", "attn"):
            fn = N._AttnHalfFused if half == "attn_fused" else N._AttnHalf
            y = fn.apply(xd, blk.norm1.weight, blk.norm1.bias, a.relative_position_bias_table, a.qkv.weight, a.qkv.bias, a.proj.weight,
                         a.proj.bias, s, heads)
        else:
            fn = N._MlpHalfFused if half == "mlp_fused" else N._MlpHalf
            y = fn.apply(xd, blk.norm2.weight, blk.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, s)
        y.backward(dy)
        N.finalize_deferred()
    torch.cuda.synchronize()
    tag = f"{half} C={Cc} defer={defer}"
    used = {n: p._pk_grad_sink for n, p in blk.named_parameters() if N.sink_written(p)}
    for n, g in used.items():
        assert not torch.isnan(g).any(), f"{tag}: NaN left in the gradient of {n}"
    seen = sorted(_check_wgrad(L, c, tag) for c in calls)
    # weight-gradient launches by operand flags (1 = row map of x, 2 = row map of g, 4 = row scale): the fused MLP half has its own slabs
    assert seen == {"attn_fused": [0, 6], "attn": [1, 6], "mlp_fused": [], "mlp": [0, 4]}[half], seen
    # float64 autograd reference of the half
    x64 = x.double().requires_grad_(True)
    P = {n: p.detach().double().requires_grad_(True) for n, p in blk.named_parameters()}
    sv = s.double().view(B, 1, 1, 1)
    if half.startswith("attn"):
        u, _ = layer_norm64(x64, P["norm1.weight"], P["norm1.bias"])
        tok, (Hp, Wp) = onet.to_windows(st_round(u))          # the LayerNorm output is a bf16 operand on both kernel paths
        out, _ = attn64(tok, P["attn.qkv.weight"], P["attn.qkv.bias"], P["attn.relative_position_bias_table"], P["attn.proj.weight"],
                        P["attn.proj.bias"], heads)
        y_ref = x64 + onet.from_windows(out, B, H, W, Hp, Wp) * sv
        names, bar = ["norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.qkv.weight", "attn.qkv.bias",
                      "attn.proj.weight", "attn.proj.bias"], 3e-2
    else:
        v, _ = layer_norm64(x64, P["norm2.weight"], P["norm2.bias"])
        y_ref = x64 + (F.gelu(st_round(v) @ P["mlp.fc1.weight"].T + P["mlp.fc1.bias"]) @ P["mlp.fc2.weight"].T + P["mlp.fc2.bias"]) * sv
        names, bar = ["norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"], 2e-2
    y_ref.backward(dy.double())
    per_sample(y.detach(), y_ref.detach(), B, f"{tag} y", 1.5e-2)
    per_sample(xd.grad, x64.grad, B, f"{tag} dx", bar)
    assert sorted(used) == sorted(names), (sorted(used), names)
    for n in names:
        e = rel(used[n], P[n].grad)
        print(f"{tag} grad {n} vs float64: {e:.3g}")
        assert e < bar, (n, e)
    for b in range(4, B, 7):
        assert torch.equal(bits(y[b]), bits(x[b])) and torch.equal(bits(xd.grad[b]), bits(dy[b])), b


# ================================================================================================ pk_reduce_many
def test_reduce_many_scalar_path_layouts_and_bounds(L, N):
    """pk_reduce_many with what the production tables never have: the scalar path (K or slab_stride not a multiple of 4, a `part` that
    is not 16-byte aligned), layouts 0 / 1 / 2, S not a multiple of 16, K not a multiple of 64, several descriptors in one launch; every
    output against the float64 slab sum ((S / 16 + 16) * U * sum|part|), and nothing written outside the K outputs of a row."""
    g = gen(900)
    pool = torch.randn(200000, generator=g, device=DEV) * 10.0 ** (torch.rand(200000, generator=g, device=DEV) * 4 - 2)
    rows, checks, off = [], [], 0
    specs = [  # part offset (floats), slab_stride, S, K, layout, T, Cin, out_stride, output size
        (0, 256, 37, 256, 0, 1, 1, 1, 256),            # vector path, S = 37
        (1, 41, 5, 37, 0, 1, 1, 3, 3 * 37),            # scalar: unaligned part, K = 37, stride 41, strided output
        (0, 216, 17, 216, 1, 9, 8, 1, 216),            # layout 1: [N = 3][T = 9][Cin = 8] -> OIHW
        (0, 32, 33, 30, 2, 20, 6, 1, 5 * 20),          # layout 2: [a < 5][b < 6] -> a * 20 + b (a column block of a 5 x 20 matrix)
        (0, 70, 200, 70, 0, 1, 1, 1, 70),              # K = 70 (70 % 4 = 2: scalar), S = 200
        (3, 132, 16, 131, 0, 1, 1, 1, 131),            # scalar: K = 131, part 12 bytes off alignment, S = 16
    ]
    for po, stride, S, K, layout, T, Cin, ostride, onum in specs:
        base = off + po
        off = -(-(base + stride * S + 64) // 4) * 4
        out = nan_t((onum + 16,))
        slabs = pool[base:base + stride * S]
        p64 = torch.stack([slabs[k * stride:k * stride + K] for k in range(S)]).double()
        i = torch.arange(K, device=DEV)
        if layout == 0:
            idx = i * ostride
        elif layout == 1:
            idx = ((i // (Cin * T)) * Cin + i % Cin) * T + (i // Cin) % T
        else:
            idx = (i // Cin) * T + (i % Cin) * ostride
        rows.append(N._row(part=(pool, base), out=(out, 0), stride=stride, S=S, K=K, layout=layout, T=T, Cin=Cin, ostride=ostride))
        checks.append((out, idx, p64.sum(0), p64.abs().sum(0), S, (stride, S, K, layout)))
    assert off <= pool.numel()
    N._reduce(rows, False, torch.device(DEV))
    torch.cuda.synchronize()
    for out, idx, ref, ab, S, spec in checks:
        ratio = float(((out[idx].double() - ref).abs() / ((-(-S // 16) + 16) * U * ab + 1e-30)).max())
        assert ratio <= 1, (spec, ratio)
        rest = torch.ones(out.numel(), dtype=torch.bool, device=DEV)
        rest[idx] = False
        assert torch.isnan(out[rest]).all(), f"{spec}: written outside the K outputs"
