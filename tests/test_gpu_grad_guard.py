"""GPU tests of the guarded optimiser step (csrc/pk_optim.hip: pk_grad_sumsq -> pk_grad_guard_finalize -> pk_adamw_step_guarded) against
the numpy restatement tests/grad_guard_np.py, which tests/test_grad_guard_host.py holds against torch on the CPU.

S = elements of one whole grid sweep (grid cap x 256 lanes x 4 elements), derived from pk_grad_sumsq_partials.  Only NaN / inf VALUES
go through ordinary arithmetic here; every index stays inside its buffer."""
import math

import numpy as np
import pytest
import torch

import grad_guard_np as gnp
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01


@pytest.fixture(scope="module")
def ops():
    from infantposeestimation_gaussianbias_amd import hipops
    return hipops


@pytest.fixture(scope="module")
def sweep(ops):
    cap = ops.grad_sumsq_partials(1 << 40)
    assert ops.grad_sumsq_partials(cap * 1024) == cap and ops.grad_sumsq_partials(cap * 1024 + 4) == cap
    return cap * 1024


def _mixed(n, seed):
    """Random gradients under flags that alternate active (2 / 3) and inactive (0 / 1) runs of 1..37 elements, starting active; the
    inactive runs hold NaN and 1e38."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    runs = rng.integers(1, 38, size=n // 10 + 2)          # mean 19: the runs cover n with a wide margin
    edges = np.minimum(np.cumsum(runs), n)
    run_of = np.searchsorted(edges, np.arange(n), side="right")
    inactive = (run_of & 1) == 1
    flags = np.where(inactive, run_of % 4 // 2, 2 + (run_of // 2) % 2).astype(np.uint8)       # inactive: 0 / 1, active: 2 / 3
    g[inactive] = np.where(np.arange(n)[inactive] % 2 == 0, np.float32(np.nan), np.float32(1e38))
    assert (flags[~inactive] & 2).all() and not (flags[inactive] & 2).any() and not inactive[0]
    return g, flags


class Guard:
    """The buffers of one guarded step over n elements."""

    def __init__(self, ops, n):
        self.ops, self.n = ops, n
        self.partials = torch.zeros(ops.grad_sumsq_partials(n), 2, dtype=torch.float64, device=DEV)
        self.state = torch.zeros(ops.GUARD_STATE_WORDS, dtype=torch.int32, device=DEV)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)

    def reduce(self, grad, flags, grad_scale, max_norm):
        self.ops.grad_sumsq(grad, flags, self.partials)
        self.ops.grad_guard_finalize(self.partials, grad_scale, max_norm, self.state, self.step_dev)

    def stats(self):
        st = self.state.cpu()
        norm, coef = st[:2].view(torch.float32).tolist()
        return norm, coef, int(st[2]), int(st[3])


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ sum of squares
def test_sumsq_matches_restatement_and_is_reproducible(ops, sweep):
    """One float4; exactly one workgroup; one float4 into a second workgroup; exactly one sweep; one float4 into the second sweep; a
    ragged third sweep.  Bound: both sides are fp64 sums of exactly representable squares (an fp32 square has 48 significant bits) in
    different orders, each within (n-1) * 2^-53 of the true sum of non-negative terms -> relative difference <= n * 2^-52."""
    S = sweep
    for k, n in enumerate((4, 1024, 1028, S, S + 4, 3 * S - 4)):
        g, flags = _mixed(n, 100 + k)
        want, bad = gnp.sumsq_np(g, flags)
        assert not bad and want > 0
        gd, fd = _up(g), _up(flags)
        G = Guard(ops, n)
        assert G.partials.shape[0] == min(-(-n // 1024), S // 1024)
        G.reduce(gd, fd, 1.0, 0.0)
        first = G.partials.clone()
        G.reduce(gd, fd, 1.0, 0.0)
        assert torch.equal(first.view(torch.int64), G.partials.view(torch.int64)), n
        p = first.cpu().numpy()
        assert (p[:, 1] == 0).all(), n
        got = float(p[:, 0].sum())
        print(f"n={n}: sumsq {got!r} restatement {want!r} rel {abs(got - want) / want:.3e} bound {n * 2.0 ** -52:.3e}")
        assert abs(got - want) <= n * 2.0 ** -52 * want, (n, got, want)
        norm, coef, skipped, total = G.stats()
        wn, wc, ws = gnp.finalize_np(got, False, 1.0, 0.0)
        # the stored norm is the fp32 rounding of sqrt(total): 2^-23 covers it and the last bits of the two fp64 totals
        assert abs(norm - wn) <= 2.0 ** -23 * wn and coef == 1.0 and (skipped, total) == (0, 0) and int(G.step_dev) == 2, (n, norm, wn)


# ------------------------------------------------------------------------------------------------ non-finite detection
def _rand_state(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=gen)
    m = torch.randn(n, device=DEV, generator=gen) * 1e-2
    v = torch.rand(n, device=DEV, generator=gen) * 1e-3
    pb = p.to(torch.bfloat16)
    return p, m, v, pb


def _guarded(ops, G, p, g, m, v, flags, pb, lr_dev, grad_scale, max_norm):
    G.reduce(g, flags, grad_scale, max_norm)
    ops.adamw_step_guarded(p, g, m, v, flags, pb, lr_dev, G.step_dev, B1, B2, EPS, WD, G.state, grad_scale)


def test_nonfinite_gradient_skips_the_whole_step(ops, sweep):
    """NaN, +inf, -inf at element 0, at element n-1 (second sweep) and at the first element of the last workgroup's range, n = S + 4."""
    n = sweep + 4
    g, flags = _mixed(n, 7)
    where = (0, n - 1, (sweep // 1024 - 1) * 1024)
    flags[list(where)] = 3
    g[list(where)] = 0.25
    fd, base = _up(flags), _up(g)
    p, m, v, pb = _rand_state(n, 8)
    keep = [t.clone() for t in (p, m, v, pb)]
    lr_dev = torch.full((1,), 1e-3, device=DEV)
    G = Guard(ops, n)
    G.step_dev.fill_(5)
    case = 0
    for at in where:
        for poison in (float("nan"), float("inf"), float("-inf")):
            case += 1
            gd = base.clone()
            gd[at] = poison
            _guarded(ops, G, p, gd, m, v, fd, pb, lr_dev, 1.0, 1.0)
            norm, coef, skipped, total = G.stats()
            assert skipped == 1 and total == case, (at, poison, skipped, total)
            assert int(G.step_dev) == 5, (at, poison)
            for name, t, k in zip("p m v bf16".split(), (p, m, v, pb), keep):
                assert torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32),
                                   k.view(torch.int16 if k.dtype == torch.bfloat16 else torch.int32)), (name, at, poison)
    # the same buffers, clean gradient: applied, counted, and the running total stays
    _guarded(ops, G, p, base, m, v, fd, pb, lr_dev, 1.0, 1.0)
    norm, coef, skipped, total = G.stats()
    assert skipped == 0 and total == 9 and int(G.step_dev) == 6 and coef < 1
    assert not torch.equal(p, keep[0]) and torch.isfinite(p).all()


def test_huge_finite_gradient_is_clipped_not_skipped(ops, sweep):
    """1e30 everywhere: every square is beyond fp32, the fp64 sum is not.  Not skipped; the norm matches the restatement to the fp32
    rounding of the stored value (2^-23 covers that rounding and the last bits of the fp64 sum and sqrt); the clipped update is finite."""
    n = sweep + 4
    g = np.full(n, 1e30, np.float32)
    flags = np.full(n, 3, np.uint8)
    p, m, v, pb = _rand_state(n, 9)
    p0 = p.clone()
    G = Guard(ops, n)
    _guarded(ops, G, p, _up(g), m, v, _up(flags), pb, torch.full((1,), 1e-3, device=DEV), 1.0, 1.0)
    norm, coef, skipped, total = G.stats()
    wn, wc, ws = gnp.finalize_np(*gnp.sumsq_np(g, flags), 1.0, 1.0)
    assert (skipped, total) == (0, 0) and not ws and int(G.step_dev) == 1
    assert math.isfinite(norm) and abs(norm - wn) <= 2.0 ** -23 * wn, (norm, wn)
    assert 0 < coef < 1 and abs(coef - wc) <= 2.0 ** -22 * wc, (coef, wc)
    for t in (p, m, v, pb.float()):
        assert torch.isfinite(t).all()
    assert not torch.equal(p, p0)


# ------------------------------------------------------------------------------------------------ pass-through
@pytest.mark.parametrize("n_extra", [1028, None])
def test_coef_one_is_bitwise_the_plain_step(ops, sweep, n_extra):
    """max_norm = 0 and max_norm = 2 x the measured norm: five steps with a changing learning rate leave p, m, v and the bf16 copy
    bitwise equal to a twin stepped by pk_adamw_step."""
    n = n_extra or sweep + 4
    g0, flags = _mixed(n, 21)
    fd = _up(flags)
    gen = torch.Generator(device=DEV).manual_seed(22)
    inactive = _up((flags & 2) == 0)
    grads = []
    for s in range(5):
        g = torch.randn(n, device=DEV, generator=gen) * (1.0 + s)
        grads.append(torch.where(inactive, _up(g0), g))           # NaN / 1e38 stay in the inactive runs
    probe = Guard(ops, n)
    probe.reduce(grads[4], fd, 0.5, 0.0)
    biggest = probe.stats()[0]
    assert math.isfinite(biggest) and biggest > 0
    lr_dev = torch.zeros(1, device=DEV)
    for max_norm in (0.0, 2.0 * biggest):
        a, b = _rand_state(n, 23), _rand_state(n, 23)
        G = Guard(ops, n)
        step_b = torch.zeros(1, dtype=torch.int32, device=DEV)
        for s, g in enumerate(grads):
            lr_dev.fill_(5e-4 * (s + 1))
            _guarded(ops, G, a[0], g, a[1], a[2], fd, a[3], lr_dev, 0.5, max_norm)
            step_b.add_(1)
            ops.adamw_step(b[0], g, b[1], b[2], fd, b[3], lr_dev, step_b, B1, B2, EPS, WD, 0.5)
            assert G.stats()[1:] == (1.0, 0, 0), (max_norm, s, G.stats())
            for name, x, y in zip("p m v".split(), a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (name, max_norm, s)
            assert torch.equal(a[3].view(torch.int16), b[3].view(torch.int16)), ("bf16", max_norm, s)
        assert int(G.step_dev) == int(step_b) == 5
        assert torch.equal(a[0][inactive].view(torch.int32), _rand_state(n, 23)[0][inactive].view(torch.int32))


# ------------------------------------------------------------------------------------------------ clipping
def test_clipped_fused_adamw_matches_restatement():
    """The model of test_fused_adamw_matches_oracle (Linear-LayerNorm-Linear plus a dead Linear), grad_scale 0.5, clip_grad_norm = half
    the first step's norm so that every step clips.  Bar: that test's 5e-6 (the same kernel arithmetic)."""
    from infantposeestimation_gaussianbias_amd import engine
    torch.manual_seed(1)
    m = torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 5)).to(DEV)
    m.add_module("dead", torch.nn.Linear(4, 4).to(DEV))
    x = torch.randn(64, 33, device=DEV)

    def backward():
        (m[2](m[1](m[0](x))) ** 2).mean().backward()
        # 'dead' never receives a gradient: after the first step its .grad is the (zero) view of an inactive slice, not None
        return {n: (None if p.grad is None or n.startswith("dead") else p.grad.detach().cpu().clone()) for n, p in m.named_parameters()}

    first = backward()
    max_norm = 0.5 * gnp.finalize_np(*gnp.sumsq_np(*gnp.flat_of(first)), 0.5, 0.0)[0]
    for p in m.parameters():
        p.grad = None
    ref = {n: p.detach().cpu().clone() for n, p in m.named_parameters()}
    dead0 = {n: v.clone() for n, v in ref.items() if n.startswith("dead")}
    st = {n: (torch.zeros_like(v), torch.zeros_like(v)) for n, v in ref.items()}
    opt = engine.FlatAdamW(m, lr=5e-4, weight_decay=WD, clip_grad_norm=max_norm)
    assert opt.guarded
    applied = 0
    for step in range(1, 6):
        opt.zero_grad()
        grads = backward()
        lr = 5e-4 * step
        opt.set_lr(lr)
        opt.step(grad_scale=0.5)
        norm, coef, skip = gnp.finalize_np(*gnp.sumsq_np(*gnp.flat_of(grads)), 0.5, max_norm)
        gs = opt.guard_stats()
        assert coef < 1 and gs["clip_coef"] < 1 and gs["skipped_last"] == 0 and gs["skipped_steps"] == 0, (step, coef, gs)
        assert abs(gs["grad_norm"] - norm) <= 1e-6 * norm and abs(gs["clip_coef"] - coef) <= 1e-6 * coef, (step, gs, norm, coef)
        applied = gnp.guarded_adamw_np(ref, grads, st, applied, lr, 0.5, coef, skip, WD)
    assert applied == 5 and int(opt.step_dev) == 5
    for n, p in m.named_parameters():
        assert rel_err(p.detach().cpu().numpy(), ref[n].numpy()) < 5e-6, n
    for n, v in dead0.items():
        assert torch.equal(dict(m.named_parameters())[n].detach().cpu(), v), n


# ------------------------------------------------------------------------------------------------ Trainer, graph and eager
CLIP = 0.05          # far below the first steps' gradient norm of the freshly initialised model (asserted: clip_coef < 1)


def _setup():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    batches = [synthetic_batch(4, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=30 + i) for i in range(3)]
    return cfg, batches


def _trainer(cfg, graph, **guard):
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    model.backbone.drop_path_rate = 0.0
    return engine.Trainer(model, cfg, iters_per_epoch=2, use_graph=graph, graph_warmup=2, **guard)


def test_trainer_clipped_graph_replay_matches_eager():
    """The setup and the bar of test_graph_replay_matches_eager_steps with the clip active: the three launches are captured with the step."""
    cfg, batches = _setup()
    traj = {}
    for graph in (False, True):
        tr = _trainer(cfg, graph, clip_grad_norm=CLIP)
        traj[graph] = [float(tr.step(batches[i % 3])["loss"].detach()) for i in range(7)]
        assert (tr._graph is not None) == graph and tr._graph_has_opt == graph
        gs = tr.opt.guard_stats()
        print(f"graph={graph}: {gs}")
        assert gs["clip_coef"] < 1 and gs["skipped_steps"] == 0 and math.isfinite(gs["grad_norm"])
        assert int(tr.opt.step_dev) == 7 == tr.opt.step_count
    assert np.allclose(traj[False], traj[True], rtol=2e-3), traj


def test_trainer_poisoned_batch_is_skipped_and_fatal_without_the_guard():
    """One NaN in `target`: the forward (and BatchNorm's running statistics) stays finite, the loss and every gradient turn NaN.  Fed as
    the 5th step of the graph run (a replay): masters and moments keep their bits, the skip is counted, training goes on.  The same
    sequence without the guard ends with non-finite parameters."""
    cfg, batches = _setup()
    poisoned = dict(batches[4 % 3])
    poisoned["target"] = poisoned["target"].clone()
    b, k = (poisoned["target_weight"].reshape(4, 17) > 0).nonzero()[0].tolist()        # a joint that counts in the loss
    poisoned["target"][b, k, 3, 5] = float("nan")
    seq = [batches[i % 3] for i in range(4)] + [poisoned] + [batches[5 % 3], batches[6 % 3]]

    tr = _trainer(cfg, True, clip_grad_norm=CLIP, skip_nonfinite=True)
    opt = tr.opt
    for b in seq[:4]:
        tr.step(b)
    assert tr._graph is not None and tr._graph_has_opt
    torch.cuda.synchronize()
    before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq)]
    loss = tr.step(seq[4])["loss"].detach().clone()
    torch.cuda.synchronize()
    assert not math.isfinite(float(loss))
    for name, t, k in zip(("flat", "exp_avg", "exp_avg_sq"), (opt.flat, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32)), name
    gs = opt.guard_stats()
    assert gs["skipped_last"] == 1 and gs["skipped_steps"] == 1 and int(opt.step_dev) == 4, gs
    losses = [float(tr.step(b)["loss"].detach()) for b in seq[5:]]
    assert all(math.isfinite(v) for v in losses), losses
    assert torch.isfinite(opt.flat).all()
    for i, p in enumerate(opt.params):
        o, k = opt.offsets[i], p.numel()
        if opt.active[i]:
            assert not torch.equal(opt.flat[o:o + k], before[0][o:o + k]), opt.names[i]
    gs = opt.guard_stats()
    assert gs["skipped_last"] == 0 and gs["skipped_steps"] == 1 and gs["clip_coef"] < 1, gs
    assert int(opt.step_dev) == 6 and opt.step_count == 7          # applied / attempted
    sd = opt.state_dict()
    assert sd["state"] and all(float(s["step"]) == 6.0 for s in sd["state"].values())

    plain = _trainer(cfg, True)
    assert not plain.opt.guarded
    for b in seq:
        plain.step(b)
    torch.cuda.synchronize()
    assert not torch.isfinite(plain.opt.flat).all()
