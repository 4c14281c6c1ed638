"""GPU tests of online hard keypoint mining (csrc/pk_loss.hip: pk_ohkm_loss_fwd / _bwd) against the float64 restatement tests/ohkm_np.py,
which tests/test_ohkm_host.py holds against the textbook torch form on the CPU.

Bounds, with u = 2^-24 (fp32 unit roundoff), all relative to the float64 value of the same float32 inputs:
  * per_map, loss: (HW + 4) u.  A term ((p - t) w)^2 carries at most 5 roundings (the difference, the product with w, and both again in
    the square); an fp32 sum of HW non-negative terms adds at most HW - 1 more in any order, the division by HW one.  (The kernel's
    order -- a few terms per thread, then a 64-lane and a 4-wave tree -- stays far below that.)  The loss adds to the largest per-map
    error only the one rounding of its double-precision finalize.
  * d_pred, per element: 4 u.  The kernel forms G scale 2 w^2 / (HW topk B) in double and rounds it once, takes p - t (one rounding)
    and multiplies (one rounding): 3 u, plus one for the second-order terms and the double rounding of the factor.  Tighter than 1e-6.
  * the selection mask is exact: every random case keeps the margin that test_ohkm_host.py asserts, 16 times the summation error.
"""
import functools
import math

import numpy as np
import pytest
import torch

import ohkm_np as onp

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = onp.U
GRAD_ULPS = 4


@pytest.fixture(scope="module")
def ops():
    from infantposeestimation_gaussianbias_amd import hipops
    return hipops


@functools.lru_cache(maxsize=None)
def _case(shape, seed):
    B, K, H, W, _ = shape
    return onp.cases(seed, B, K, H, W)


@functools.lru_cache(maxsize=None)
def _ref(shape, seed, weighted, scale):
    """The float64 reference of one case, computed once and shared (read-only) by the tests that need it."""
    pred, target, weight = _case(shape, seed)
    out = onp.ohkm_np(pred, target, weight if weighted else None, shape[4], scale)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(ops, pred, target, weight, topk, scale, counts=None, grad_out=None):
    """-> loss (python float), per_map, mask, d_pred as host arrays; `grad_out`: the upstream gradient of the scalar loss."""
    p = G(pred).requires_grad_(True)
    w = None if weight is None else G(weight)
    loss, per_map, mask = ops.ohkm_loss(p, G(target), w, topk, scale, counts, return_selection=True)
    assert loss.shape == () and loss.dtype == torch.float32 and per_map.shape == mask.shape == pred.shape[:2] and mask.dtype == torch.uint8
    assert not per_map.requires_grad and not mask.requires_grad
    (dp,) = torch.autograd.grad(loss, p, None if grad_out is None else torch.tensor(grad_out, device=DEV))
    return loss.detach().cpu().numpy(), per_map.cpu().numpy(), mask.cpu().numpy(), dp.cpu().numpy()


def _assert_parity(got, ref, hw, tag):
    loss, per_map, mask, dp = got
    rl, rpm, rmask, rg = ref
    assert np.array_equal(mask, rmask), tag
    e_map = np.abs(per_map - rpm) / np.where(rpm == 0, 1.0, rpm)
    e_loss = abs(float(loss) - rl) / abs(rl)
    e_grad = np.abs(dp - rg) / np.where(rg == 0, 1.0, np.abs(rg))
    print(f"{tag}: per_map {e_map.max() / U:.2f} u, loss {e_loss / U:.2f} u (bound {hw + 4} u), d_pred {e_grad.max() / U:.2f} u (bound {GRAD_ULPS} u)")
    assert e_map.max() <= (hw + 4) * U and e_loss <= (hw + 4) * U, tag
    assert e_grad.max() <= GRAD_ULPS * U, tag
    assert not dp[mask == 0].any(), tag                                    # exactly zero (and written) on unselected maps
    assert np.array_equal(dp == 0, rg == 0), tag


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", onp.SHAPES)
def test_parity_with_the_float64_restatement(ops, shape, weighted, scale):
    B, K, H, W, topk = shape
    for seed in onp.case_seeds(shape, weighted):
        pred, target, weight = _case(shape, seed)
        weight = weight if weighted else None
        ref = _ref(shape, seed, weighted, scale)
        _assert_parity(_run(ops, pred, target, weight, topk, scale), ref, H * W, f"{shape} seed {seed} weighted={weighted} scale={scale}")
    # an upstream gradient other than 1 scales d_pred (same bound: it enters the factor that is rounded once), and changes nothing else
    got = _run(ops, pred, target, weight, topk, scale, grad_out=-3.0)
    _assert_parity(got, ref[:3] + (-3.0 * ref[3],), H * W, f"{shape} upstream gradient -3")


# ------------------------------------------------------------------------------------------------ 2. exact arithmetic, ties
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_exact_case_is_bitwise_float64_and_ties_fall_to_the_lower_index(ops, scale):
    pred, target, weight, topk = onp.exact_case()
    rl, rpm, rmask, rg = onp.ohkm_np(pred, target, weight, topk, scale)
    loss, per_map, mask, dp = _run(ops, pred, target, weight, topk, scale)
    assert np.array_equal(per_map.view(np.uint32), rpm.astype(np.float32).view(np.uint32))
    assert np.float32(loss).view(np.uint32) == np.float32(rl).view(np.uint32) and float(np.float32(rl)) == rl
    assert np.array_equal(mask, rmask)
    assert mask.tolist() == [[0, 1, 1, 1, 0, 0, 0, 1], [1, 0, 0, 1, 0, 1, 0, 1], [1, 1, 1, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 1, 1, 1]]
    # the factor scale 2 / (64 * 4 * 4) is a power of two here, so the gradient is exact as well (as values: the restatement's zeros on
    # unselected maps carry the sign of p - t, the kernel stores +0 there)
    assert np.array_equal(dp, rg.astype(np.float32)) and not np.signbit(dp[mask == 0]).any()


# ------------------------------------------------------------------------------------------------ 3. topk = K is the pixel loss
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("shape", [s for s in onp.SHAPES if s[4] == s[1]])
def test_topk_equal_k_is_the_pixel_loss_kind_0(ops, shape, weighted):
    """Same tensors through pk_pixel_loss (kind 0): equal loss and gradient within the bounds of test 1.  (Both kernels take the same
    rounded p - t and each adds two roundings -- the factor and the product -- so the gradients lie within 4 u of each other.)"""
    B, K, H, W, topk = shape
    pred, target, weight = _case(shape, 0)
    weight = weight if weighted else None
    loss, _, mask, dp = _run(ops, pred, target, weight, topk, 1.0)
    p = G(pred).requires_grad_(True)
    pl = ops.pixel_loss(p, G(target), None if weight is None else G(weight), 0)
    (pg,) = torch.autograd.grad(pl, p)
    pl, pg = float(pl.detach()), pg.cpu().numpy()
    e_loss = abs(float(loss) - pl) / pl
    e_grad = np.abs(dp - pg) / np.where(pg == 0, 1.0, np.abs(pg))
    print(f"{shape} weighted={weighted}: loss {e_loss / U:.2f} u, gradient {e_grad.max() / U:.2f} u")
    assert mask.all() and e_loss <= (H * W + 4) * U and e_grad.max() <= GRAD_ULPS * U and np.array_equal(dp == 0, pg == 0)


# ------------------------------------------------------------------------------------------------ 4. NaN
@pytest.mark.parametrize("weighted", [True, False])
def test_one_nan_makes_the_loss_nan_and_selects_that_map(ops, weighted):
    shape, seed = onp.SHAPES[1], 0                                # (5, 17, 9, 3, 8)
    B, K, H, W, topk = shape
    pred, target, weight = _case(shape, seed)
    weight = weight if weighted else None
    clean = _ref(shape, seed, weighted, 1.0)[2]
    b, k = 2, int(np.flatnonzero(clean[2] == 0)[-1])             # a map that is NOT among the selected ones without the NaN
    poisoned = pred.copy()
    poisoned[b, k, 4, 1] = np.nan
    loss, per_map, mask, dp = _run(ops, poisoned, target, weight, topk, 1.0)
    assert math.isnan(float(loss)) and math.isnan(per_map[b, k]) and mask[b, k] == 1
    others = [i for i in range(B) if i != b]
    assert np.array_equal(mask[others], clean[others]) and np.isfinite(np.delete(per_map, b, 0)).all()
    assert np.array_equal(mask, onp.ohkm_np(poisoned, target, weight, topk, 1.0)[2])          # sample b: the NaN first, then its 7 largest
    assert np.isfinite(dp[others]).all() and not dp[mask == 0].any()


# ------------------------------------------------------------------------------------------------ 5. counts, repeatability
def test_counts_accumulate_and_two_runs_give_the_same_bits(ops):
    for shape in (onp.SHAPES[0], onp.SHAPES[2], onp.SHAPES[3]):
        B, K, H, W, topk = shape
        counts = torch.zeros(K, dtype=torch.int64, device=DEV)
        want = np.zeros(K, np.int64)
        for seed in onp.case_seeds(shape, True):
            pred, target, weight = _case(shape, seed)
            first = _run(ops, pred, target, weight, topk, 0.5, counts)
            want += _ref(shape, seed, True, 0.5)[2].sum(0, dtype=np.int64)
        assert counts.cpu().numpy().tolist() == want.tolist() and want.sum() == 3 * B * topk
        again = _run(ops, pred, target, weight, topk, 0.5)          # the last case once more, without counts
        for a, b in zip(first, again):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert counts.cpu().numpy().tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------ 6. models
def _with_grad(model):
    return {n for n, p in model.named_parameters() if p.grad is not None}


def _batch(cfg, B, seed):
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    return synthetic_batch(B, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=seed)


def _model(cfg, **kw):
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    torch.manual_seed(0)
    m = PoseEstimator(cfg.model.backbone, 17, False, cfg.model.head_type, True, **kw).to(DEV).train()
    m.backbone.drop_path_rate = 0.0
    return m


def _np_loss(out, batch, topk, scale):
    hm = out["heatmaps"].detach().float().cpu().numpy()
    w = batch["target_weight"].cpu().numpy().reshape(hm.shape[:2])
    return onp.ohkm_np(hm, batch["target"].cpu().numpy(), w, topk, scale), hm[0, 0].size


def test_heatmap_head_model_runs_the_mined_loss_through_its_padded_twin():
    from infantposeestimation_gaussianbias_amd import dispatch
    from infantposeestimation_gaussianbias_amd.configs import get_config
    cfg = get_config("hrnet_w18")
    batch = _batch(cfg, 4, 41)
    plain, mined = _model(cfg), _model(cfg, ohkm_topk=8)
    outs = {}
    for name, m in (("plain", plain), ("mined", mined)):
        outs[name] = m(batch["img"], batch["target"], batch["target_weight"])
        outs[name]["loss"].backward()
    tw = dispatch.padded_twin(mined)
    assert tw is not None and tw.twin.loss_fn.ohkm_topk == 8                       # the twin is what runs, and it mines
    (rl, _, rmask, _), hw = _np_loss(outs["mined"], batch, 8, 1.0)
    got = float(outs["mined"]["loss"].detach())
    print(f"hrnet_w18 twin: loss {got} restatement {rl} ({abs(got - rl) / rl / U:.2f} u, bound {hw + 4} u), plain {float(outs['plain']['loss'].detach())}")
    assert abs(got - rl) <= (hw + 4) * U * rl
    assert mined.selection_counts().tolist() == rmask.sum(0).tolist() and plain.selection_counts() is None
    # every parameter the plain loss reaches receives a gradient (the rest are the dead fuse layers of the last module, as before)
    assert _with_grad(mined) == _with_grad(plain) and len(_with_grad(mined)) > 0.9 * len(list(mined.parameters()))
    assert all(torch.isfinite(p.grad).all() for p in mined.parameters() if p.grad is not None)


def test_fusion_model_adds_the_term_and_is_bit_identical_with_mining_off():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.models import FusionPoseLoss
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    batch = _batch(cfg, 4, 43)
    models = {"default": _model(cfg), "off": _model(cfg, ohkm_topk=0, ohkm_weight=1.0), "on": _model(cfg, ohkm_topk=8, ohkm_weight=0.5)}
    outs = {}
    for name, m in models.items():
        outs[name] = m(batch["img"], batch["target"], batch["target_weight"], batch["keypoints"], input_size=cfg.data.input_size)
        outs[name]["loss"].backward()
    # off == built without the arguments, bit for bit: losses and every gradient
    assert list(outs["off"]["losses"]) == list(FusionPoseLoss.NAMES) == list(outs["default"]["losses"])
    for n in FusionPoseLoss.NAMES:
        assert torch.equal(outs["off"]["losses"][n].view(torch.int32), outs["default"]["losses"][n].view(torch.int32)), n
    grads = {k: dict((n, p.grad) for n, p in m.named_parameters()) for k, m in models.items()}
    assert _with_grad(models["off"]) == _with_grad(models["default"]) == _with_grad(models["on"])
    for n, g in grads["default"].items():
        if g is not None:
            assert torch.equal(g.view(torch.int32), grads["off"][n].view(torch.int32)), n
    # on: the seventh term is ohkm_weight * OHKM of the model's own heatmaps, and the total is the sum of the seven named parts
    lo = outs["on"]["losses"]
    assert list(lo) == list(FusionPoseLoss.NAMES[:6]) + ["ohkm_loss", "total_loss"]
    (rl, _, rmask, _), hw = _np_loss(outs["on"], batch, 8, 0.5)
    got = float(lo["ohkm_loss"].detach())
    print(f"hrformer_small: ohkm_loss {got} restatement {rl} ({abs(got - rl) / rl / U:.2f} u, bound {hw + 4} u)")
    assert abs(got - rl) <= (hw + 4) * U * rl
    total = np.float32(0)
    for n in list(FusionPoseLoss.NAMES[:6]) + ["ohkm_loss"]:
        total = np.float32(total + np.float32(float(lo[n].detach())))
    assert float(lo["total_loss"].detach()) == float(total) == float(outs["on"]["loss"].detach())
    for n in FusionPoseLoss.NAMES[:6]:                                     # the six fused terms are untouched by the switch
        assert torch.equal(lo[n].view(torch.int32), outs["default"]["losses"][n].view(torch.int32)), n
    assert models["on"].selection_counts().tolist() == rmask.sum(0).tolist()
    changed = [n for n, g in grads["on"].items() if g is not None and not torch.equal(g, grads["default"][n])]
    assert len(changed) > 0.5 * len(_with_grad(models["on"])) and all(torch.isfinite(g).all() for g in grads["on"].values() if g is not None)


# ------------------------------------------------------------------------------------------------ 7. graph replay
CLIP = 0.05          # as tests/test_gpu_grad_guard.py: far below the first steps' gradient norm


def _setup():
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    cfg.model.ohkm_topk = 8
    batches = [synthetic_batch(4, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=30 + i) for i in range(3)]
    return cfg, batches


def _trainer(cfg, graph, **guard):
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    model.backbone.drop_path_rate = 0.0
    return engine.Trainer(model, cfg, iters_per_epoch=2, use_graph=graph, graph_warmup=2, **guard)


def test_trainer_graph_replay_with_mining_matches_eager():
    """The setup and the bar of test_trainer_clipped_graph_replay_matches_eager with cfg.model.ohkm_topk = 8: the selection, its mask and
    the counts live inside the captured step (optimiser included), and every one of the 7 steps selects 8 joints per sample."""
    cfg, batches = _setup()
    traj, terms = {}, {}
    for graph in (False, True):
        tr = _trainer(cfg, graph, clip_grad_norm=CLIP)
        assert tr.model.loss_fn.ohkm_topk == 8
        traj[graph] = []
        for i in range(7):
            out = tr.step(batches[i % 3])
            traj[graph].append(float(out["loss"].detach()))                    # read per step: a replay rewrites the same tensors
        assert (tr._graph is not None) == graph and tr._graph_has_opt == graph
        counts = tr.model.selection_counts()
        print(f"graph={graph}: counts {counts.tolist()}")
        assert counts.sum() == 7 * 4 * 8 and counts.max() <= 7 * 4
        assert int(tr.opt.step_dev) == 7 == tr.opt.step_count
        terms[graph] = float(out["losses"]["ohkm_loss"].detach())
    assert np.allclose(traj[False], traj[True], rtol=2e-3) and np.isclose(terms[False], terms[True], rtol=2e-3), (traj, terms)
