"""Gradient attribution on the device: pk_stem_dgrad, pk_nhwc_bf16_to_nchw_f32, pk_saliency_reduce and pk_gradcam against their float64
restatement (tests/attribution_np.py) at the sizes where the kernels' loops change behaviour, then the batched pass through two models
(hrnet_w18: heatmap head, padded twin; hrformer_small: fusion head): against plain autograd bit for bit, chunk size by chunk size, against
the bf16-aware oracle with the oracle's own sensitivity as the yardstick, its side effects, and the surface above it (SensitivityAnalyzer,
GradCAMVisualizer, PoseInference, the --saliency_map / --grad_cam paths of inference.py)."""
import argparse
import functools

import numpy as np
import pytest
import torch

import attribution_np as anp
from recipe import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
JOINTS = (0, 5, 16)
SIZE = (1, 3, 128, 96)


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached inputs are read-only


def bits(t):
    """bf16 device tensor -> uint16 numpy."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def from_bits(u16):
    """uint16 numpy -> bf16 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).to(DEV).view(BF16)


def _bf16_values(rng, shape, scale=1.0):
    """Random values that are bf16 numbers, as float64."""
    return anp.bf16_round(scale * rng.standard_normal(shape))


# ------------------------------------------------------------------------------------------------ pk_stem_dgrad
# (B, Hs, Ws, Cout, c_real): the issue's five shapes on the RGB path (c_real <= 4: 8-byte weight reads), and the 16-byte path at 5 and 8
STEM = [(2, 10, 6, 64, 3), (1, 9, 7, 64, 3), (3, 1, 1, 8, 3), (1, 2, 5, 16, 3), (2, 33, 25, 64, 3), (1, 9, 7, 64, 4), (1, 9, 7, 64, 5),
        (1, 9, 7, 64, 8)]


@pytest.mark.parametrize("case", STEM)
def test_stem_dgrad_against_the_restatement(case):
    """Bar, derived: one bf16 rounding of the result (2^-8 relative, half an ulp would be 2^-9) plus an fp32 sum of at most 4 Cout exact
    products, each addition off by at most 2^-24 of the running magnitude, which the sum of |terms| bounds."""
    from infantposeestimation_gaussianbias_amd import hipops
    B, Hs, Ws, Cout, c_real = case
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    rng = np.random.default_rng(Hs * 1000 + Ws * 10 + c_real)
    g, w = _bf16_values(rng, (B, Ho, Wo, Cout)), _bf16_values(rng, (Cout, 9, 8), 0.2)      # pad channels of the pack hold values too
    want, mag = anp.stem_dgrad(g, w, Hs, Ws, c_real)
    got = hipops.stem_dgrad(G(g, BF16), G(w, BF16), (Hs, Ws), c_real)
    assert got.dtype == BF16 and tuple(got.shape) == (B, Hs, Ws, 8)
    got_bits = bits(got)
    assert not got_bits[..., c_real:].any()                                               # exactly +0
    got = got.double().cpu().numpy()
    bound = 2.0 ** -8 * np.abs(want) + 4 * Cout * 2.0 ** -24 * mag
    worst = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print(f"stem_dgrad {case}: worst |got - want| / bound = {worst:.3f}")
    assert (np.abs(got - want) <= bound).all() and want[..., :c_real].any()


def test_stem_dgrad_refusals():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)
    with pytest.raises(PoseKernelError, match="gives 5 x 3"):
        hipops.stem_dgrad(z(2, 6, 3, 64), z(64, 9, 8), (10, 6))                            # wrong Ho
    with pytest.raises(PoseKernelError, match="Cout=12"):
        hipops.stem_dgrad(z(2, 5, 3, 12), z(12, 9, 8), (10, 6))
    with pytest.raises(PoseKernelError, match="c_real=9"):
        hipops.stem_dgrad(z(2, 5, 3, 64), z(64, 9, 8), (10, 6), 9)
    with pytest.raises(PoseKernelError, match="forward pack"):
        hipops.stem_dgrad(z(2, 5, 3, 64), z(3, 9, 64), (10, 6))                            # the data-gradient pack's shape
    with pytest.raises(PoseKernelError, match="bfloat16"):
        hipops.stem_dgrad(z(2, 5, 3, 64).float(), z(64, 9, 8), (10, 6))


# ------------------------------------------------------------------------------------------------ unpack and saliency
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 9, 7), (3, 33, 25)])
def test_unpack_and_saliency_bit_for_bit(shape):
    from infantposeestimation_gaussianbias_amd import hipops
    B, H, W = shape
    rng = np.random.default_rng(B * 100 + H)
    b = (anp.bf16_round(rng.standard_normal(shape + (8,))).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    flat = b.reshape(-1, 8)
    flat[0, :3] = [0x8000, 0x0000, 0x8000]                                                # -0, +0, -0: the maximum is +0
    if len(flat) > 4:
        flat[1, :3] = [0x4000, 0xc000, 0x3f80]                                            # equal magnitudes of both signs
        flat[2, 1] = 0x7fc0                                                               # a NaN in a real channel
        flat[3, 0], flat[3, 2] = 0xffc0, 0x7f80                                           # a negative NaN next to +inf
        flat[4, 3:] = 0x7fc0                                                              # NaNs in the pad channels only
    x = from_bits(b)
    sal, want = hipops.saliency_reduce(x, 3), anp.saliency(b, 3)
    assert sal.dtype == torch.float32 and tuple(sal.shape) == shape
    got = sal.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert got.reshape(-1)[0] == 0.0 and not np.signbit(got.reshape(-1)[0])
    if len(flat) > 4:
        f = got.reshape(-1)
        assert f[1] == 2.0 and np.isnan(f[2]) and np.isnan(f[3]) and np.isfinite(f[4])
    for c_real in (1, 8):
        got = hipops.saliency_reduce(x, c_real).cpu().numpy()
        want = anp.saliency(b, c_real)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    for C, Cp in ((3, 8), (8, 8), (1, 8)):
        got = hipops.packed_grad_to_nchw(x, C)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, C, H, W)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), anp.nhwc_to_nchw(b, C).view(np.uint32))       # NaN payloads and -0 included
    wide = np.concatenate([b, b[..., ::-1]], axis=-1)                                     # Cpad = 16, C = 11: a second, partly used chunk
    got = hipops.packed_grad_to_nchw(from_bits(wide), 11)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), anp.nhwc_to_nchw(wide, 11).view(np.uint32))


# ------------------------------------------------------------------------------------------------ pk_gradcam
CAM = [(1, 1, 1, 8, 8), (3, 5, 7, 32, 32), (2, 16, 12, 24, 18), (1, 64, 48, 32, 32), (17, 12, 9, 256, 256)]


def _cam_check(got, want, Gv, hw, where=""):
    """The bars: maps within 2^-22 absolute (values in [0,1], one fp32 rounding of a float64 result, headroom for the order of the float64
    sums); weights within 2^-23 relative plus 1e-12 sum|G| / (h w); range within 1e-12 relative."""
    cam, wts, rng = (t.cpu().numpy() for t in got)
    cam_w, wts_w, rng_w = want
    d_cam = float(np.abs(cam.astype(np.float64) - cam_w).max())
    tol_w = 2.0 ** -23 * np.abs(wts_w.astype(np.float64)) + 1e-12 * np.abs(Gv).sum(axis=(1, 2))[:, :wts_w.shape[1]] / hw
    d_w = float((np.abs(wts.astype(np.float64) - wts_w) / np.maximum(tol_w, 1e-300)).max())
    d_r = float((np.abs(rng - rng_w) / np.maximum(np.abs(rng_w), 1e-300)).max())
    print(f"grad_cam {where}: map diff {d_cam:.3g} (bar {2.0 ** -22:.3g}), weights diff / bar {d_w:.3g}, range relative diff {d_r:.3g} (bar 1e-12)")
    assert d_cam <= 2.0 ** -22 and d_w <= 1.0 and d_r <= 1e-12


@pytest.mark.parametrize("case", CAM)
def test_grad_cam_against_the_restatement(case):
    from infantposeestimation_gaussianbias_amd import hipops
    B, h, w, C, c_used = case
    rng = np.random.default_rng(h * 100 + C)
    A, Gv = _bf16_values(rng, (B, h, w, C)), _bf16_values(rng, (B, h, w, C), 0.05)
    got = hipops.grad_cam(G(A, BF16), G(Gv, BF16), c_used)
    assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (B, h, w) and tuple(got[1].shape) == (B, c_used)
    assert got[2].dtype == torch.float64 and tuple(got[2].shape) == (B, 2)
    _cam_check(got, anp.grad_cam(A, Gv, c_used), Gv, h * w, str(case))
    cam = got[0].cpu().numpy()
    assert cam.min() >= 0.0 and cam.max() <= 1.0
    if h * w > 1:
        assert all(cam[b].max() > 0.99 for b in range(B))                                 # normalised per sample, not over the batch
    if c_used < C:                                                                        # garbage beyond c_used changes nothing
        A2, G2 = A.copy(), Gv.copy()
        A2[..., c_used:], G2[..., c_used:] = np.nan, 1e30
        other = hipops.grad_cam(G(A2, BF16), G(G2, BF16), c_used)
        assert all(torch.equal(a, b) for a, b in zip(got, other))
    again = hipops.grad_cam(G(A, BF16), G(Gv, BF16), c_used)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                             # fixed order: the same bits


def test_grad_cam_special_cases():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    rng = np.random.default_rng(9)
    B, h, w, C = 4, 5, 7, 16
    A, Gv = _bf16_values(rng, (B, h, w, C)), _bf16_values(rng, (B, h, w, C), 0.05)
    A[1], Gv[1] = np.abs(A[1]), -np.abs(Gv[1])                                            # the weighted sum is negative everywhere
    A[2], Gv[2] = 1.0, 0.5                                                                # a constant positive map
    plain = [t.clone() for t in hipops.grad_cam(G(A, BF16), G(Gv, BF16))]
    _cam_check(plain, anp.grad_cam(A, Gv), Gv, h * w, "special")
    assert not plain[0][1].any() and not plain[0][2].any() and plain[2][1].tolist() == [0.0, 0.0] and plain[2][2].tolist() == [8.0, 8.0]
    for which in ("activation", "gradient"):
        A2, G2 = A.copy(), Gv.copy()
        (A2 if which == "activation" else G2)[3, 2, 3, 5] = np.nan                        # one NaN in sample 3
        cam, wts, rng_ = hipops.grad_cam(G(A2, BF16), G(G2, BF16))
        assert torch.isnan(cam[3]).all() and torch.isnan(rng_[3]).all(), which
        assert torch.equal(cam[:3], plain[0][:3]) and torch.equal(rng_[:3], plain[2][:3]) and torch.equal(wts[:3], plain[1][:3]), which
        assert bool(torch.isnan(wts[3]).any()) == (which == "gradient")
    z = torch.zeros(1, 4, 4, 8, dtype=BF16, device=DEV)
    with pytest.raises(PoseKernelError, match="c_used=9"):
        hipops.grad_cam(z, z, 9)
    with pytest.raises(PoseKernelError, match="must both be"):
        hipops.grad_cam(z, z[:, :2])


# ------------------------------------------------------------------------------------------------ models
_SPEC = {"hrnet_w18": ("hrnet_w18", "heatmap", "hrnet_w18_heatmap", 41), "hrformer_small": ("hrformer_small", "fusion", "hrformer_small_fusion", 40)}
MODELS = ["hrnet_w18", "hrformer_small"]


def _keys(name):
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        return json.load(f)[_SPEC[name][2]]


@functools.lru_cache(maxsize=None)
def _model(name):
    """As tests/test_gpu_occlusion.py builds them: synthetic weights, eval mode."""
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    bb, head, _, salt = _SPEC[name]
    m = PoseEstimator(bb, 17, False, head, True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(_keys(name), salt).items()}, strict=True)
    return m.to(DEV).eval()


def _input():
    return G(synth_input("attribution", SIZE))


@functools.lru_cache(maxsize=None)
def _single(name):
    """attribution_maps one joint at a time: what every other chunking is compared with.  Read-only."""
    from infantposeestimation_gaussianbias_amd import utils
    return utils.attribution_maps(_model(name), _input(), joints=JOINTS, batch_size=1)


def _same(a, b):
    layer = a["layers"][0]
    return (a["layers"] == b["layers"] and torch.equal(a["saliency"], b["saliency"]) and torch.equal(a["grad"], b["grad"])
            and torch.equal(a["cams"][layer], b["cams"][layer]) and torch.equal(a["cam_weights"][layer], b["cam_weights"][layer])
            and torch.equal(a["cam_range"][layer], b["cam_range"][layer]) and torch.equal(a["base"], b["base"]))


@pytest.mark.parametrize("name", MODELS)
def test_plain_autograd_reaches_the_input_and_equals_the_batched_pass(name):
    """1. `x.requires_grad_(); model(x)['heatmaps'][0, k].sum().backward()` fills x.grad (empty before this feature), and the batched
    pass at batch_size 1 gives the same bits."""
    from infantposeestimation_gaussianbias_amd import hipops
    m, res = _model(name), _single(name)
    H, W = SIZE[2:]
    assert tuple(res["saliency"].shape) == (3, H, W) and tuple(res["grad"].shape) == (3, 3, H, W) and res["saliency"].dtype == torch.float32
    try:
        for i, k in enumerate(JOINTS):
            x = _input().requires_grad_()
            hm = m(x)["heatmaps"]
            hm[0, k].sum().backward()
            assert x.grad is not None and tuple(x.grad.shape) == SIZE and bool(x.grad.any())
            assert torch.equal(x.grad[0], res["grad"][i]), k
            assert torch.equal(x.grad[0].abs().amax(0), res["saliency"][i]), k
            assert torch.equal(hipops.heatmap_summary(hm.detach())[0, k], res["base"][i])
    finally:
        m.zero_grad(set_to_none=True)                             # the plain path fills the parameters' .grad, as autograd does
    assert len({res["saliency"][i].cpu().numpy().tobytes() for i in range(3)}) == 3       # the joints differ


@pytest.mark.parametrize("name", MODELS)
def test_chunk_size_does_not_change_a_bit(name):
    """2. Chunks of 2 and 1, of 3, and one chunk of at most 64 give the bits of one joint at a time: in eval mode every data-gradient kernel
    works per sample.  The (3,H,W) and the packed input likewise."""
    from infantposeestimation_gaussianbias_amd import nnops, utils
    m, x, one = _model(name), _input(), _single(name)
    layer = one["layers"][0]
    assert layer.endswith("fuse_layers.0") and tuple(one["cam_range"][layer].shape) == (3, 2) and tuple(one["base"].shape) == (3, 4)
    h, w = one["cams"][layer].shape[1:]
    assert (h, w) == (SIZE[2] // 4, SIZE[3] // 4) and one["cam_weights"][layer].shape[1] == {"hrnet_w18": 18, "hrformer_small": 32}[name]
    for bs in (2, 3, 64):
        assert _same(utils.attribution_maps(m, x, joints=JOINTS, batch_size=bs), one), bs
    assert _same(utils.attribution_maps(m, x[0], joints=list(JOINTS), batch_size=2), one)
    assert _same(utils.attribution_maps(m, nnops.to_features(x), joints=JOINTS, batch_size=3), one)
    sal_only = utils.attribution_maps(m, x, joints=JOINTS, target_layers=(), batch_size=3)
    assert sal_only["cams"] == {} and sal_only["layers"] == [] and torch.equal(sal_only["saliency"], one["saliency"])
    every = utils.attribution_maps(m, x, target_layers=layer)                              # joints=None: all 17, the default chunk
    assert tuple(every["saliency"].shape) == (17,) + SIZE[2:] and torch.equal(every["saliency"][list(JOINTS)], one["saliency"])
    assert torch.equal(every["cams"][layer][list(JOINTS)], one["cams"][layer])


@functools.lru_cache(maxsize=None)
def _oracle(name, dithered):
    """The bf16-aware oracle (oracle.nets.pose_forward's two lines with Ctx(train=False, q=bf16_storage), the backbone's output kept for
    its gradient): per joint one autograd.grad with the graph retained.  -> saliency (3,H,W) and CAM (3,h,w), float64 numpy."""
    from oracle import nets as onet
    P32 = {k: torch.from_numpy(v).clone() for k, v in synth_state_dict(_keys(name), _SPEC[name][3]).items()}
    x = torch.from_numpy(synth_input("attribution", SIZE))
    if dithered:
        x = x * (1 + 1e-5 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)))
    x.requires_grad_(True)
    P, ctx = onet.bf16_weights(P32), onet.Ctx(train=False, q=onet.bf16_storage)
    feat = onet.backbone(x, P, ctx)
    hm = onet.fusion_head(feat, P, ctx)["heatmaps"] if "head.fusion_weight" in P else onet.heatmap_head(feat, P)
    sal, cam = [], []
    for k in JOINTS:
        gx, gf = torch.autograd.grad(hm[0, k].sum(), [x, feat], retain_graph=True)
        sal.append(gx[0].abs().amax(0).double().numpy())
        cam.append(anp.grad_cam_literal(feat.detach().double().numpy(), gf.double().numpy())[0, 0])
    return np.stack(sal), np.stack(cam)


def _l2(a, b):
    """|a - b| / |b|.  A map that is 0 everywhere (a CAM whose weighted sum is negative everywhere: hrnet_w18's joint 16 with the synthetic
    weights) has no relative distance: equal maps are 0 apart, anything else infinitely far -- there the check asks for equality."""
    num, den = float(np.linalg.norm((a - b).ravel())), float(np.linalg.norm(b.ravel()))
    return num / den if den > 0.0 else (0.0 if num == 0.0 else float("inf"))


@pytest.mark.parametrize("name", MODELS)
def test_maps_against_the_bf16_aware_oracle(name):
    """3. Per joint d = |HIP - O| / |O| (L2) of the saliency maps, and of the default layer's CAM, at most 2 d0; d0 = the same distance
    between the oracle's map and the oracle's map of the input dithered by x (1 + 1e-5 n): two independently rounded bf16 runs, expected to
    be about as far apart as HIP and the oracle are (the yardstick and the margin of test_hrformer_small_expected_gradient_vs_bf16_aware_
    oracle).  Measured on an MI355X: DESIGN.md "Gradient attribution", Checks."""
    res = _single(name)
    layer = res["layers"][0]
    (sal_o, cam_o), (sal_p, cam_p) = _oracle(name, False), _oracle(name, True)
    sal_h, cam_h = res["saliency"].double().cpu().numpy(), res["cams"][layer].double().cpu().numpy()
    rows = []
    for i, k in enumerate(JOINTS):
        rows.append((k, _l2(sal_h[i], sal_o[i]), _l2(sal_p[i], sal_o[i]), _l2(cam_h[i], cam_o[i]), _l2(cam_p[i], cam_o[i])))
        print(f"{name} joint {k}: saliency d {rows[-1][1]:.4f} d0 {rows[-1][2]:.4f}; CAM d {rows[-1][3]:.4f} d0 {rows[-1][4]:.4f}")
    for k, d_s, d0_s, d_c, d0_c in rows:
        assert d_s <= 2 * d0_s, (name, k, "saliency", d_s, d0_s)
        assert d_c <= 2 * d0_c, (name, k, "cam", d_c, d0_c)


@pytest.mark.parametrize("name", MODELS)
def test_side_effects(name):
    """4. Parameter gradients stay None (the real model's; a twin's are not scattered), the input is not marked, a later forward is
    unchanged, nothing is left for a later step; training mode and an unknown layer raise."""
    from infantposeestimation_gaussianbias_amd import nnops, utils
    m, x = _model(name), _input()
    m.zero_grad(set_to_none=True)
    with torch.no_grad():
        before = m(x)["heatmaps"].clone()
    assert all(p.grad is None for p in m.parameters())
    res = utils.attribution_maps(m, x, joints=JOINTS, batch_size=2)
    assert all(p.grad is None for p in m.parameters())
    assert not x.requires_grad and x.grad is None
    assert not nnops._PENDING                                     # the postponed slab reductions of that backward were dropped
    tw = getattr(m, "_pk_twin", None)
    assert bool(tw) == (name == "hrnet_w18")
    if tw:
        assert not tw._pending
    with torch.no_grad():
        assert torch.equal(m(x)["heatmaps"], before)
    assert _same(res, _single(name))
    y = x.clone().requires_grad_()                                # a caller's tensor that already requires grad keeps an empty .grad
    utils.attribution_maps(m, y, joints=[5], target_layers=())
    assert y.requires_grad and y.grad is None
    m.train()
    try:
        with pytest.raises(RuntimeError, match="needs eval mode"):
            utils.attribution_maps(m, x)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="no tapped layer named 'backbone.nowhere'") as e:
        utils.attribution_maps(m, x, joints=[0], target_layers="backbone.nowhere")
    assert "backbone.bn1" in str(e.value) and res["layers"][0] in str(e.value)            # the message lists the tapped names
    with pytest.raises(ValueError, match="outside 0 .. 16"):
        utils.attribution_maps(m, x, joints=[17])
    with pytest.raises(ValueError, match="one image"):
        utils.attribution_maps(m, torch.cat([x, x]))
    assert all(p.grad is None for p in m.parameters()) and not nnops._PENDING
    # another layer: a conv + BatchNorm + ReLU output early in the network, and two layers at once
    two = utils.attribution_maps(m, x, joints=[5], target_layers=["backbone.bn2", res["layers"][0]], batch_size=1)
    assert two["layers"] == ["backbone.bn2", res["layers"][0]] and tuple(two["cams"]["backbone.bn2"].shape) == (1, SIZE[2] // 4, SIZE[3] // 4)
    assert torch.equal(two["cams"][res["layers"][0]][0], res["cams"][res["layers"][0]][1])


def test_the_reference_calls():
    """5. compute_input_sensitivity, generate_cam with and without a joint."""
    from infantposeestimation_gaussianbias_amd import hipops, nnops, utils
    name = "hrnet_w18"
    m, x, res = _model(name), _input(), _single(name)
    layer = res["layers"][0]
    one = utils.SensitivityAnalyzer.compute_input_sensitivity(m, x, 5)
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == SIZE[2:]
    assert np.array_equal(one, res["saliency"][1].cpu().numpy()) and one.any() and not x.requires_grad
    viz = utils.GradCAMVisualizer(m, layer)
    cam = viz.generate_cam(x, 5)
    assert cam.is_cuda and tuple(cam.shape) == (1, 1) + tuple(res["cams"][layer].shape[1:]) and torch.equal(cam[0, 0], res["cams"][layer][1])
    assert torch.equal(utils.GradCAMVisualizer(m).generate_cam(x, 5), cam)                # None: the same default layer
    # target_class=None: the sum of all joints' maps, here through plain autograd under the collector on the same model
    collector = utils.GradientCollector(m, [layer])
    try:
        with nnops.observe(collector):
            hm = m(x.clone().requires_grad_())["heatmaps"]
        hm[0].sum().backward()
        A, Gr, c_used = collector.pairs()[layer]
        want = hipops.grad_cam(A, Gr, c_used)[0][:, None]
    finally:
        m.zero_grad(set_to_none=True)
    assert c_used == 18 and A.shape[-1] == 24
    got = viz.generate_cam(x)
    assert tuple(got.shape) == tuple(cam.shape) and torch.equal(got, want) and not torch.equal(got, cam)
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------ front end
@functools.lru_cache(maxsize=None)
def _pose():
    import inference
    torch.manual_seed(11)
    return inference.PoseInference(config="hrnet_w18", flip_test=False)


def test_pose_inference_attributes_the_crop_of_predict():
    from infantposeestimation_gaussianbias_amd import utils
    pose = _pose()
    img = np.random.default_rng(12).integers(0, 256, (120, 160, 3)).astype(np.uint8)
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    res = pose.attribution(img, bbox, joints=[5, 2])
    x, c, s = pose.preprocess(img, bbox)
    want = utils.attribution_maps(pose.model, x, joints=[5, 2])
    w, h = pose.input_size
    assert tuple(res["saliency"].shape) == (2, h, w) and _same(res, want) and bool(res["saliency"].any())
    assert np.array_equal(res["center"], c) and np.array_equal(res["scale"], s)
    one = pose.attribution(img, bbox, joints=2, target_layers=())
    assert torch.equal(one["saliency"][0], want["saliency"][1]) and one["cams"] == {}


@pytest.mark.parametrize("flag", ["saliency_map", "grad_cam"])
def test_attribution_switches_draw_where_the_crop_lies(flag, tmp_path, capsys):
    import inference
    from PIL import Image
    pose = _pose()
    img = np.random.default_rng(12).integers(0, 256, (120, 160, 3)).astype(np.uint8)
    bbox = np.array([60.0, 30.0, 120.0, 100.0])
    out = tmp_path / f"{flag}.png"
    args = argparse.Namespace(saliency_map=None, grad_cam=None, grad_cam_layer=None, output=str(out))
    setattr(args, flag, 5)
    res = inference.main_attribution(args, pose, img, bbox)
    text = capsys.readouterr().out
    heat = res["saliency"][0] if flag == "saliency_map" else res["cams"][res["layers"][0]][0]
    top = int(torch.argmax(heat.reshape(-1)))
    assert f"(x {top % heat.shape[1]}, y {top // heat.shape[1]})" in text and "joint 5" in text
    assert ("Input saliency" in text) == (flag == "saliency_map") and ("Grad-CAM" in text and res["layers"][0] in text) == (flag == "grad_cam")
    drawn = np.asarray(Image.open(out).convert("RGB"))[:, :, ::-1]
    assert drawn.shape == img.shape
    changed = (drawn != img).any(-1)
    assert changed.any() and not changed[:, :10].any() and not changed[:5].any()          # only where the crop lies
    with pytest.raises(SystemExit):
        inference.main_attribution(argparse.Namespace(**{**vars(args), flag: 17}), pose, img, bbox)
