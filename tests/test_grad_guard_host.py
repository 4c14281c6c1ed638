"""Host-side checks of the guarded optimiser step (no GPU): the numpy restatement the GPU tests compare the kernels with
(tests/grad_guard_np.py) is itself held against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in float64 on the CPU; the header
declares the entry points; train.py takes the two flags."""
import numpy as np
import pytest
import torch

import grad_guard_np as gnp
from conftest import rel_err
from oracle import optim as oopt

GRAD_SCALE, LR, WD, STEPS = 0.5, 3e-3, 0.01, 4


def _model():
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.LayerNorm(17), torch.nn.Linear(17, 5)).double()


def _first_norm():
    g = torch.Generator().manual_seed(11)
    grads = {n: torch.randn(p.shape, generator=g, dtype=torch.float64) for n, p in _model().named_parameters()}
    return GRAD_SCALE * float(np.sqrt(gnp.sumsq_np(*gnp.flat_of(grads, torch.float64))[0]))


@pytest.mark.parametrize("case", ["clip_active", "clip_inactive", "off"])
def test_restatement_matches_torch_clip_and_adamw(case):
    """Two parameter groups (decay / no decay, train.py:55-97), random gradients, STEPS steps with a changing learning rate.  Everything
    in float64 (device_casts=False): the clip coefficient agrees to 1e-12 and the parameters to float64 round-off (1e-12 norm-wise: a
    few hundred operations per element at 1.1e-16 each, through Adam's well-conditioned m / sqrt(v))."""
    max_norm = {"clip_active": 0.5 * _first_norm(), "clip_inactive": 1e3 * _first_norm(), "off": 0.0}[case]
    m = _model()
    named = list(m.named_parameters())
    topt = torch.optim.AdamW([{"params": [p for n, p in named if not oopt.is_no_decay(n)], "weight_decay": WD},
                              {"params": [p for n, p in named if oopt.is_no_decay(n)], "weight_decay": 0.0}],
                             lr=LR, betas=(0.9, 0.999), eps=1e-8)
    assert all(len(g["params"]) > 0 for g in topt.param_groups)
    ref = {n: p.detach().clone() for n, p in named}
    state = {n: (torch.zeros_like(p), torch.zeros_like(p)) for n, p in ref.items()}
    gen = torch.Generator().manual_seed(11)
    applied, coefs = 0, []
    for step in range(1, STEPS + 1):
        lr = LR * step
        grads = {n: torch.randn(p.shape, generator=gen, dtype=torch.float64) * step for n, p in named}
        # torch: scale (the 1/world averaging), clip, step
        for n, p in named:
            p.grad = grads[n] * GRAD_SCALE
        if max_norm > 0:
            total_norm = float(torch.nn.utils.clip_grad_norm_([p for _, p in named], max_norm))
            want_coef = min(1.0, max_norm / (total_norm + 1e-6))
        else:
            want_coef = 1.0
        for g in topt.param_groups:
            g["lr"] = lr
        topt.step()
        # restatement
        total, nonfinite = gnp.sumsq_np(*gnp.flat_of(grads, torch.float64))
        norm, coef, skip = gnp.finalize_np(total, nonfinite, GRAD_SCALE, max_norm, device_casts=False)
        assert not skip
        assert abs(coef - want_coef) <= 1e-12, (step, coef, want_coef)
        if max_norm > 0:
            assert abs(norm - total_norm) <= 1e-12 * total_norm
        applied = gnp.guarded_adamw_np(ref, grads, state, applied, lr, GRAD_SCALE, coef, skip, WD, device_casts=False)
        coefs.append(coef)
    assert applied == STEPS
    assert all(c < 1 for c in coefs) if case == "clip_active" else all(c == 1.0 for c in coefs), coefs
    for n, p in named:
        assert rel_err(p.detach().numpy(), ref[n].numpy()) < 1e-12, n


def test_restatement_casts_skip_and_masking():
    """The device variant rounds norm and coef to fp32; inactive elements are ignored even when they hold NaN; an active inf/NaN sets the
    flag without any arithmetic on it; a skipped step changes nothing and does not count."""
    g = np.array([3.0, np.nan, 4.0, 1e38], np.float32)
    total, bad = gnp.sumsq_np(g, np.array([2, 0, 3, 1], np.uint8))
    assert total == 25.0 and not bad
    norm, coef, skip = gnp.finalize_np(total, bad, 0.5, 1.0)
    assert norm == 2.5 and coef == float(np.float32(1.0 / (2.5 + 1e-6))) and not skip
    assert gnp.finalize_np(total, bad, 0.5, 3.0)[1] == 1.0 and gnp.finalize_np(total, bad, 0.5, float("inf"))[1] == 1.0
    for poison in (np.nan, np.inf, -np.inf):
        g2 = g.copy()
        g2[2] = poison
        assert gnp.sumsq_np(g2, np.array([2, 0, 3, 1], np.uint8))[1]
    assert not gnp.sumsq_np(np.full(8, 1e30, np.float32), np.full(8, 2, np.uint8))[1]      # squares beyond fp32, still finite
    p = {"w": torch.ones(3)}
    st = {"w": (torch.zeros(3), torch.zeros(3))}
    assert gnp.guarded_adamw_np(p, {"w": torch.ones(3)}, st, 7, 1e-3, 1.0, 1.0, True, 0.01) == 7
    assert torch.equal(p["w"], torch.ones(3)) and not st["w"][0].any()
    assert gnp.guarded_adamw_np(p, {"w": torch.ones(3)}, st, 7, 1e-3, 1.0, 1.0, False, 0.01) == 8
    assert not torch.equal(p["w"], torch.ones(3))


def test_header_declares_guard_entry_points():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_grad_sumsq_partials", 1), ("pk_grad_sumsq", 6), ("pk_grad_guard_finalize", 7), ("pk_adamw_step_guarded", 16)):
        assert name in decl, name
        assert len(decl[name][1]) == n_args, (name, len(decl[name][1]))
        assert hasattr(_lib.lib, name)
    assert len(decl["pk_adamw_step_guarded"][1]) == len(decl["pk_adamw_step"][1]) + 1
    L = _lib.lib
    # the grid is a function of n only: ceil(n / 4 / 256) workgroups up to a cap
    assert [L.pk_grad_sumsq_partials(n) for n in (4, 1024, 1028, 2048, 2052)] == [1, 1, 2, 2, 3]
    cap = L.pk_grad_sumsq_partials(1 << 40)
    assert L.pk_grad_sumsq_partials(cap * 1024) == cap and L.pk_grad_sumsq_partials(cap * 1024 - 4) == cap
    assert L.pk_grad_sumsq_partials((cap - 1) * 1024) == cap - 1
    assert L.pk_grad_sumsq_partials(0) < 0 and L.pk_grad_sumsq_partials(6) < 0
    # argument checks run before anything touches a device
    buf = (np.zeros(64, np.float64)).ctypes.data
    assert L.pk_grad_sumsq(buf, buf, 1028, buf, 1, None) != 0 and b"n_partials" in L.pk_last_error_string()
    assert L.pk_grad_guard_finalize(buf, 0, 1.0, 0.0, buf, buf, None) != 0


def test_train_parser_has_guard_flags_off_by_default():
    import train
    p = train.build_parser()
    a = p.parse_args([])
    assert a.clip_grad_norm == 0.0 and a.skip_nonfinite is False
    a = p.parse_args(["--config", "hrformer_small", "--graph", "--clip_grad_norm", "1.0", "--skip_nonfinite"])
    assert a.clip_grad_norm == 1.0 and a.skip_nonfinite is True and a.graph


def test_flat_adamw_rejects_bad_clip_value():
    from infantposeestimation_gaussianbias_amd import engine
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            engine.FlatAdamW(torch.nn.Linear(2, 2), clip_grad_norm=bad)
