"""GPU tests of the weight EMA kept by the fused AdamW step (csrc/pk_optim.hip: pk_adamw_step_ema) against the numpy restatement
tests/ema_np.py, which tests/test_ema_host.py holds against the closed form of the average.

S = elements of one whole grid sweep (grid cap x 256 lanes x 4 elements), derived from pk_grad_sumsq_partials as in
test_gpu_grad_guard.py, whose `_mixed` flag pattern is re-created here.  Only NaN / inf VALUES go through ordinary arithmetic; every index
stays inside its buffer.

U = 2^-24, the fp32 unit round-off.  Per-step bound on an active element: |e_dev - e_ref| <= BOUND U M with M = max(|p_new|, |e_prev|) and
e_ref the float64 restatement advanced from the device's own e_prev and p_new.  With w = 1 - d_t <= 9/11 (t >= 1) and |p - e| <= 2 M:
  fp32 d_t (one rounding of the quotient, or of ema_decay) and fp32 w (one more): |dw| <= 2 U, times |p - e|          <= 4    U M
  the subtraction p - e rounds by U |p - e|, carried through w                                                         <= 1.64 U M
  the product w (p - e) rounds by U w |p - e|                                                                          <= 1.64 U M
  the final sum lies between e and p, so it rounds by                                                                  <= 1    U M
together 8.3 U M; the library is built without FMA contraction (which could only lower that).  BOUND = 9 (a looser count of the same
roundings gives 16); the largest ratio measured on the MI355X is 3.01 (n = S + 4), and against the fp32 variant of the restatement every
element of every case was bitwise equal."""
import math

import numpy as np
import pytest
import torch

import ema_np

pytestmark = pytest.mark.gpu
DEV = "cuda"
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01
U = 2.0 ** -24
DECAY = 0.999
BOUND = 9


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


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _rand_state(n, seed):
    """p, m, v, the bf16 copy, and an average half a unit away from p (so that a wrong decay shows far above the rounding bound)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    p = torch.randn(n, device=DEV, generator=gen)
    m = torch.randn(n, device=DEV, generator=gen) * 1e-2
    v = torch.rand(n, device=DEV, generator=gen) * 1e-3
    e = p + 0.5 * torch.randn(n, device=DEV, generator=gen)
    return p, m, v, p.to(torch.bfloat16), e


class Guard:
    """The buffers of one guarded step over n elements (test_gpu_grad_guard.py's)."""

    def __init__(self, ops, n):
        self.ops = ops
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


def _ema_step(ops, G, step_dev, p, g, m, v, flags, pb, e, lr_dev, grad_scale, max_norm=0.0, decay=DECAY):
    """One step through pk_adamw_step_ema: behind the two guard launches when G is given, else after the host-side step count."""
    if G is not None:
        G.reduce(g, flags, grad_scale, max_norm)
        ops.adamw_step_ema(p, g, m, v, flags, pb, lr_dev, G.step_dev, B1, B2, EPS, WD, G.state, e, decay, grad_scale)
    else:
        step_dev.add_(1)
        ops.adamw_step_ema(p, g, m, v, flags, pb, lr_dev, step_dev, B1, B2, EPS, WD, None, e, decay, grad_scale)


def _five_grads(n, flags, g0):
    gen = torch.Generator(device=DEV).manual_seed(22)
    inactive = _up((flags & 2) == 0)
    return [torch.where(inactive, _up(g0), torch.randn(n, device=DEV, generator=gen) * (1.0 + s)) for s in range(5)], inactive


SIZES = [4, 1024, 1028, None]          # None: S + 4 (one float4 into the second sweep)


# ------------------------------------------------------------------------------------------------ 1. the masters
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("n_or_sweep", SIZES)
def test_masters_are_bitwise_those_of_the_plain_step(ops, sweep, n_or_sweep, guarded):
    """Five steps with a changing learning rate, guard_state NULL and a real guard with coef == 1 (max_norm 0): p, m, v and the bf16 copy
    are bitwise equal to a twin stepped by pk_adamw_step."""
    n = n_or_sweep or sweep + 4
    g0, flags = _mixed(n, 21)
    fd = _up(flags)
    grads, _ = _five_grads(n, flags, g0)
    a, b = _rand_state(n, 23), _rand_state(n, 23)
    G = Guard(ops, n) if guarded else None
    step_a = torch.zeros(1, dtype=torch.int32, device=DEV)
    step_b = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.zeros(1, device=DEV)
    for s, g in enumerate(grads):
        lr_dev.fill_(5e-4 * (s + 1))
        _ema_step(ops, G, step_a, a[0], g, a[1], a[2], fd, a[3], a[4], lr_dev, 0.5)
        step_b.add_(1)
        ops.adamw_step(b[0], g, b[1], b[2], fd, b[3], lr_dev, step_b, B1, B2, EPS, WD, 0.5)
        if guarded:
            assert G.stats()[1:] == (1.0, 0, 0), (s, G.stats())
        for name, x, y in zip("p m v bf16".split(), a[:4], b[:4]):
            assert torch.equal(_bits(x), _bits(y)), (name, n, guarded, s)
    assert int(G.step_dev if guarded else step_a) == int(step_b) == 5
    assert not torch.equal(a[4], b[4])          # ... and the average did move


# ------------------------------------------------------------------------------------------------ 2. the average
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("n_or_sweep", SIZES)
def test_ema_matches_restatement_step_by_step(ops, sweep, n_or_sweep, guarded):
    """After every one of the five steps: the float64 restatement, advanced from the device's previous e and new p, within BOUND U of the
    larger operand on every active element (module docstring); inactive elements keep the bits of the initial average.
    Measured on the MI355X: see DESIGN.md, "Weight EMA"."""
    n = n_or_sweep or sweep + 4
    g0, flags = _mixed(n, 21)
    fd = _up(flags)
    active = (flags & 2) != 0
    grads, _ = _five_grads(n, flags, g0)
    p, m, v, pb, e = _rand_state(n, 23)
    e0 = e.cpu().numpy().copy()
    G = Guard(ops, n) if guarded else None
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.zeros(1, device=DEV)
    worst = exact = 0.0
    for s, g in enumerate(grads):
        e_prev = e.cpu().numpy().copy()
        lr_dev.fill_(5e-4 * (s + 1))
        _ema_step(ops, G, step_dev, p, g, m, v, fd, pb, e, lr_dev, 0.5)
        p_new, e_dev = p.cpu().numpy(), e.cpu().numpy()
        want = ema_np.ema_update_np(e_prev, p_new, s + 1, DECAY, flags)
        scale = np.maximum(np.abs(p_new), np.abs(e_prev))[active]
        err = np.abs(e_dev.astype(np.float64) - want)[active]
        worst = max(worst, float((err / (U * scale)).max()))
        fp32 = ema_np.ema_update_np(e_prev, p_new, s + 1, DECAY, flags, device_casts=True)
        exact += float((fp32.view(np.uint32) == e_dev.view(np.uint32)).mean()) / 5
        assert (err <= BOUND * U * scale).all(), (n, guarded, s, float((err / (U * scale)).max()))
        assert np.array_equal(e_dev.view(np.uint32)[~active], e0.view(np.uint32)[~active]), (n, guarded, s)
        assert not np.array_equal(e_dev[active], e_prev[active])
    print(f"n={n} guarded={guarded}: worst |e_dev - e_ref| = {worst:.3f} U max(|p_new|, |e_prev|) (bound {BOUND}); "
          f"share bitwise equal to the fp32 restatement {exact:.6f}")


# ------------------------------------------------------------------------------------------------ 3. skipped step
def test_skipped_step_freezes_the_ema(ops, sweep):
    """NaN, +inf, -inf at element 0, at element n-1 (second sweep) and at the first element of the last workgroup's range, n = S + 4: ema,
    p, m, v, the bf16 copy and step_dev keep their bits; a clean gradient afterwards moves the average."""
    n = sweep + 4
    g, flags = _mixed(n, 7)
    where = (0, n - 1, (sweep // 1024 - 1) * 1024)
    flags[list(where)] = 3
    g[list(where)] = 0.25
    fd, base = _up(flags), _up(g)
    p, m, v, pb, e = _rand_state(n, 8)
    keep = [t.clone() for t in (p, m, v, pb, e)]
    lr_dev = torch.full((1,), 1e-3, device=DEV)
    G = Guard(ops, n)
    G.step_dev.fill_(5)
    case = 0
    for at in where:
        for poison in (float("nan"), float("inf"), float("-inf")):
            case += 1
            gd = base.clone()
            gd[at] = poison
            _ema_step(ops, G, None, p, gd, m, v, fd, pb, e, lr_dev, 1.0, max_norm=1.0)
            norm, coef, skipped, total = G.stats()
            assert skipped == 1 and total == case and int(G.step_dev) == 5, (at, poison, skipped, total)
            for name, t, k in zip("p m v bf16 ema".split(), (p, m, v, pb, e), keep):
                assert torch.equal(_bits(t), _bits(k)), (name, at, poison)
    _ema_step(ops, G, None, p, base, m, v, fd, pb, e, lr_dev, 1.0, max_norm=1.0)
    norm, coef, skipped, total = G.stats()
    assert skipped == 0 and total == 9 and int(G.step_dev) == 6 and coef < 1
    active = _up((flags & 2) != 0)
    assert not torch.equal(p, keep[0]) and torch.isfinite(p).all()
    assert (e[active] != keep[4][active]).float().mean() > 0.99 and torch.isfinite(e).all()
    assert torch.equal(_bits(e[~active]), _bits(keep[4][~active]))


# ------------------------------------------------------------------------------------------------ 4. the decay
def test_decay_follows_step_dev(ops):
    """step_dev = 1, then 2: the two launches together give what 2/11, then 3/12 give (two per-step bounds; the first one's error is
    carried through a factor d_2 < 1).  step_dev = 10^6: exactly ema_decay, far from what the warm-up formula would still give there."""
    n = 1028
    g0, flags = _mixed(n, 31)
    fd = _up(flags)
    active = (flags & 2) != 0
    gd = torch.where(_up(~active), _up(g0), torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(32)))
    p, m, v, pb, e = _rand_state(n, 33)
    lr_dev = torch.full((1,), 1e-3, device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    e0 = e.cpu().numpy().astype(np.float64)

    def launch(t):
        step_dev.fill_(t)
        ops.adamw_step_ema(p, gd, m, v, fd, pb, lr_dev, step_dev, B1, B2, EPS, WD, None, e, DECAY, 1.0)
        return p.cpu().numpy().astype(np.float64), e.cpu().numpy().astype(np.float64)

    p1, e1 = launch(1)
    p2, e2 = launch(2)
    r1 = e0 + (1.0 - 2.0 / 11.0) * (p1 - e0)
    r2 = r1 + (1.0 - 3.0 / 12.0) * (p2 - r1)
    scale = np.maximum.reduce([np.abs(p1), np.abs(p2), np.abs(e0), np.abs(r1)])
    err = (np.abs(e2 - r2) / (U * scale))[active]
    print(f"two launches: worst {err.max():.3f} U (bound {2 * BOUND})")
    assert (err <= 2 * BOUND).all(), err.max()
    p3, e3 = launch(10 ** 6)
    r3 = e2 + (1.0 - DECAY) * (p3 - e2)
    scale = np.maximum(np.abs(p3), np.abs(e2))
    err = (np.abs(e3 - r3) / (U * scale))[active]
    print(f"step_dev = 10^6: worst {err.max():.3f} U (bound {BOUND})")
    assert (err <= BOUND).all(), err.max()
    warm = e2 + (1.0 - (1.0 + 1e6) / (10.0 + 1e6)) * (p3 - e2)
    assert (np.abs(e3 - warm) > BOUND * U * scale)[active].mean() > 0.9          # the warm-up value would miss the bound
    assert np.array_equal(e3[~active], e0[~active])


# ------------------------------------------------------------------------------------------------ 5. Trainer, eager and graph
CLIP = 0.05          # far below the first steps' gradient norm of the freshly initialised model (asserted: clip_coef < 1)


def _setup():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    batches = [synthetic_batch(4, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=30 + i) for i in range(3)]
    return cfg, batches


def _trainer(cfg, graph, **kw):
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    model.backbone.drop_path_rate = 0.0
    return engine.Trainer(model, cfg, iters_per_epoch=2, use_graph=graph, graph_warmup=2, ema_decay=DECAY, **kw)


def _poisoned(batch):
    """One NaN in `target` (test_gpu_grad_guard.py): the forward stays finite, the loss and every gradient turn NaN."""
    bad = dict(batch)
    bad["target"] = bad["target"].clone()
    b, k = (bad["target_weight"].reshape(4, 17) > 0).nonzero()[0].tolist()
    bad["target"][b, k, 3, 5] = float("nan")
    return bad


class _Follow:
    """The float64 restatement next to a Trainer: advanced from the masters copied to the host after every step."""

    def __init__(self, opt):
        torch.cuda.synchronize()
        self.opt = opt
        self.e = opt.ema.cpu().numpy().astype(np.float64)
        assert np.array_equal(self.e, opt.flat.cpu().numpy().astype(np.float64))
        self.scale = np.abs(self.e)
        self.applied = 0

    def advance(self):
        torch.cuda.synchronize()
        p = self.opt.flat.cpu().numpy().astype(np.float64)
        self.applied += 1
        self.scale = np.maximum.reduce([self.scale, np.abs(p), np.abs(self.e)])
        self.e = ema_np.ema_update_np(self.e, p, self.applied, DECAY, self.opt.flags.cpu().numpy())

    def check(self, steps):
        """steps per-step bounds add up (every d_t <= 1 contracts the earlier errors), each taken at the largest operand seen."""
        torch.cuda.synchronize()
        got = self.opt.ema.cpu().numpy().astype(np.float64)
        active = (self.opt.flags.cpu().numpy() & 2) != 0
        ok = self.scale > 0
        ratio = np.abs(got - self.e)[ok] / (U * self.scale[ok])
        assert np.array_equal(got[~ok], self.e[~ok])
        assert np.array_equal(got[~active], self.opt.flat.cpu().numpy().astype(np.float64)[~active])      # never updated, never averaged
        assert not np.array_equal(got[active], self.opt.flat.cpu().numpy().astype(np.float64)[active])
        return float(ratio.max()), steps * BOUND


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_ema_matches_restatement(graph):
    """hrformer_small, 96 x 128, B = 4, seven steps (graph mode: two eager, the capture, four more replays, d_t different at each): at the
    end opt.ema lies within 7 x BOUND U max|.| of the restatement (measured: 2.05).  A decay frozen at capture would be 4/13 at steps 4..7 instead of
    5/14 .. 8/17: off by up to 0.16 |p - e|."""
    cfg, batches = _setup()
    tr = _trainer(cfg, graph)
    assert tr.opt.ema is not None and tr.opt.ema.data_ptr() != tr.opt.flat.data_ptr() and not tr.opt.guarded
    ref = _Follow(tr.opt)
    for i in range(7):
        tr.step(batches[i % 3])
        ref.advance()
    assert (tr._graph is not None) == graph and tr._graph_has_opt == graph
    assert int(tr.opt.step_dev) == 7 == tr.opt.step_count
    worst, bound = ref.check(7)
    print(f"graph={graph}: worst |ema - restatement| = {worst:.3f} U max|.| (bound {bound})")
    assert worst <= bound


def test_trainer_guarded_poisoned_step_freezes_the_ema():
    """The same run in graph mode with clip_grad_norm = 0.05, skip_nonfinite and the poisoned batch as step 5 (a replay): opt.ema keeps
    its bits across that step and moves at the next; the restatement, advanced on the six applied updates only (t = applied updates),
    still holds at the end."""
    cfg, batches = _setup()
    seq = [batches[i % 3] for i in range(4)] + [_poisoned(batches[4 % 3])] + [batches[5 % 3], batches[6 % 3]]
    tr = _trainer(cfg, True, clip_grad_norm=CLIP, skip_nonfinite=True)
    opt = tr.opt
    ref = _Follow(opt)
    for b in seq[:4]:
        tr.step(b)
        ref.advance()
    assert tr._graph is not None and tr._graph_has_opt
    before = [t.clone() for t in (opt.ema, opt.flat)]
    loss = tr.step(seq[4])["loss"].detach().clone()
    torch.cuda.synchronize()
    assert not math.isfinite(float(loss))
    assert torch.equal(_bits(opt.ema), _bits(before[0])) and torch.equal(_bits(opt.flat), _bits(before[1]))
    gs = opt.guard_stats()
    assert gs["skipped_last"] == 1 and gs["skipped_steps"] == 1 and int(opt.step_dev) == 4, gs
    tr.step(seq[5])
    ref.advance()
    assert not torch.equal(opt.ema, before[0]) and torch.isfinite(opt.ema).all()
    tr.step(seq[6])
    ref.advance()
    gs = opt.guard_stats()
    assert gs["skipped_steps"] == 1 and gs["clip_coef"] < 1 and int(opt.step_dev) == 6 and opt.step_count == 7, gs
    worst, bound = ref.check(7)
    print(f"guarded graph run: worst |ema - restatement| = {worst:.3f} U max|.| (bound {bound})")
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ 6. the swap
def test_ema_weights_swaps_contents_between_graph_replays():
    """Two trainers from the same seed over the same seven batches, graph mode.  One of them evaluates under ema_weights() after step 4:
    inside, model.inference gives bitwise what a fresh model loaded with ema_state_dict() gives, and not what the raw weights give;
    after it, flat and ema have their bits back and the model trains on; an exception inside still swaps back; after step 7 masters,
    moments and average are bitwise those of the trainer that never swapped."""
    from infantposeestimation_gaussianbias_amd.models import build_model
    cfg, batches = _setup()
    img = batches[1]["img"]
    b = _trainer(cfg, True)
    for i in range(7):
        b.step(batches[i % 3])
    torch.cuda.synchronize()
    a = _trainer(cfg, True)
    for i in range(4):
        a.step(batches[i % 3])
    assert a._graph is not None and a._graph_has_opt and a.model.training
    torch.cuda.synchronize()
    flat0, ema0 = a.opt.flat.clone(), a.opt.ema.clone()
    ptrs = (a.opt.flat.data_ptr(), a.opt.ema.data_ptr())
    fresh = build_model(cfg).to(DEV).eval()
    fresh.load_state_dict(a.opt.ema_state_dict())
    kp_ema, sc_ema = [t.clone() for t in fresh.inference(img, flip=False)]
    fresh.load_state_dict(a.model.state_dict())
    kp_raw, sc_raw = [t.clone() for t in fresh.inference(img, flip=False)]
    with a.ema_weights() as m:
        assert m is a.model and not a.model.training
        assert torch.equal(_bits(a.opt.flat), _bits(ema0)) and torch.equal(_bits(a.opt.ema), _bits(flat0))
        kp, sc = [t.clone() for t in a.model.inference(img, flip=False)]
    assert torch.equal(_bits(kp), _bits(kp_ema)) and torch.equal(_bits(sc), _bits(sc_ema))
    assert not (torch.equal(kp, kp_raw) and torch.equal(sc, sc_raw))
    assert a.model.training and ptrs == (a.opt.flat.data_ptr(), a.opt.ema.data_ptr())
    assert torch.equal(_bits(a.opt.flat), _bits(flat0)) and torch.equal(_bits(a.opt.ema), _bits(ema0))
    with pytest.raises(ZeroDivisionError):
        with a.ema_weights():
            1 / 0
    assert a.model.training
    assert torch.equal(_bits(a.opt.flat), _bits(flat0)) and torch.equal(_bits(a.opt.ema), _bits(ema0))
    a.model.eval()
    with a.ema_weights():
        pass
    assert not a.model.training          # the mode found is the mode restored
    a.model.train()
    for i in range(4, 7):
        a.step(batches[i % 3])
    torch.cuda.synchronize()
    for name in ("flat", "exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(_bits(getattr(a.opt, name)), _bits(getattr(b.opt, name))), name
    assert not torch.equal(a.opt.flat, flat0)


# ------------------------------------------------------------------------------------------------ 7. checkpoint round trip
def test_ema_state_dict_round_trip():
    """Linear-LayerNorm-Linear plus BatchNorm1d: ema_state_dict has the model's keys and shapes, averaged parameters and LIVE running
    statistics; load_ema_state_dict into a second optimiser reproduces ema bitwise; reset_ema makes ema the masters, bitwise."""
    from infantposeestimation_gaussianbias_amd import engine

    def make():
        torch.manual_seed(1)
        return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 5), torch.nn.BatchNorm1d(5)).to(DEV)

    m = make()
    x = torch.randn(64, 33, device=DEV)
    opt = engine.FlatAdamW(m, lr=5e-3, weight_decay=WD, ema_decay=0.9)
    assert torch.equal(opt.ema, opt.flat)
    for step in range(3):
        opt.zero_grad()
        (m(x) ** 2).mean().backward()
        opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(opt.ema, opt.flat)
    sd, live = opt.ema_state_dict(), m.state_dict()
    assert list(sd) == list(live) and all(sd[k].shape == live[k].shape and sd[k].dtype == live[k].dtype for k in sd)
    for n, p, o in zip(opt.names, opt.params, opt.offsets):
        assert torch.equal(_bits(sd[n].reshape(-1)), _bits(opt.ema[o:o + p.numel()])), n
    assert not torch.equal(sd["0.weight"], live["0.weight"]) and not torch.equal(sd["3.weight"], live["3.weight"])
    for k in ("3.running_mean", "3.running_var", "3.num_batches_tracked"):
        assert torch.equal(sd[k], live[k]) and sd[k].data_ptr() != live[k].data_ptr(), k
    assert int(sd["3.num_batches_tracked"]) == 3 and not torch.equal(live["3.running_mean"], torch.zeros(5, device=DEV))
    other = engine.FlatAdamW(make(), ema_decay=0.9)
    assert not torch.equal(other.ema, opt.ema)
    other.load_ema_state_dict({k: v.cpu() for k, v in sd.items()})
    assert torch.equal(_bits(other.ema), _bits(opt.ema))
    opt.reset_ema()
    assert torch.equal(_bits(opt.ema), _bits(opt.flat))
