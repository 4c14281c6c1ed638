"""Occlusion sensitivity on the device: pk_occlude_batch, pk_heatmap_summary and pk_occlusion_paint bit for bit against their numpy
restatement (tests/occlusion_np.py) at the sizes where the kernels' loops change behaviour, then the sweep through two models
(hrnet_w18: heatmap head, padded twin; hrformer_small: fusion head) against single forwards of torch-made occluded inputs summarised and
painted by the restatement, and the surface above it (SensitivityAnalyzer, PoseInference, the --occlusion_map path of inference.py)."""
import argparse
import functools

import numpy as np
import pytest
import torch

import occlusion_np as onp
from recipe import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

# (H, W, patch, stride): 12 x 10 = 120 pixels, fewer than one workgroup; 33 x 25: a ragged tail and a patch that does not divide;
# 20 x 15: stride > patch (gaps); 17 x 40: a single row of positions
SHAPES = [(12, 10, 4, 3), (33, 25, 7, 3), (20, 15, 4, 8), (17, 40, 16, 8)]
FILL = (0.3, -1.7, 2.05)                                          # none of them a bf16 value


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached inputs are read-only


def bits(t):
    """bf16 device tensor -> uint16 numpy."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _image(H, W):
    a = np.random.default_rng(H * 100 + W).standard_normal((3, H, W)).astype(np.float32)
    a.setflags(write=False)
    return a


def _packed(H, W):
    from infantposeestimation_gaussianbias_amd import nnops
    x = nnops.to_features(G(_image(H, W))[None])
    assert np.array_equal(bits(x[0]), onp.pack_image(_image(H, W)))
    return x


# ------------------------------------------------------------------------------------------------ pk_occlude_batch
@pytest.mark.parametrize("fill", [None, FILL])
@pytest.mark.parametrize("shape", SHAPES)
def test_occlude_batch_equals_the_restatement_bitwise(shape, fill):
    from infantposeestimation_gaussianbias_amd import hipops
    H, W, p, s = shape
    x = _packed(H, W)
    before = x.clone()
    got = hipops.occlude_batch(x, p, s, fill=fill)
    want = onp.occluded_copies(onp.pack_image(_image(H, W)), p, s, fill)
    ny, nx = onp.grid(H, W, p, s)
    assert tuple(got.shape) == (ny * nx, H, W, 8) and got.dtype == torch.bfloat16 and len(want) == ny * nx
    assert np.array_equal(bits(got), want)
    assert not bits(got)[..., 3:].any()                           # pad channels, inside the patch as well
    assert torch.equal(x.view(torch.int16), before.view(torch.int16))          # the source is unchanged
    assert np.array_equal(bits(hipops.occlude_batch(x[0], p, s, fill=fill)), want)      # (H,W,8) is the same call
    if fill is not None:                                          # the fill is rounded as the input conversion rounds
        assert np.array_equal(bits(got)[0, 0, 0, :3], onp.bf16_bits(np.array(FILL, np.float32)))


def test_occlude_batch_window_and_bounds():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    H, W, p, s = SHAPES[1]
    x = _packed(H, W)
    whole = hipops.occlude_batch(x, p, s)
    P = whole.shape[0]
    assert P == 54
    part = hipops.occlude_batch(x, p, s, first=5, n=7)
    assert tuple(part.shape) == (7, H, W, 8) and torch.equal(part.view(torch.int16), whole[5:12].view(torch.int16))
    last = hipops.occlude_batch(x, p, s, first=P - 1, n=1)
    assert torch.equal(last.view(torch.int16), whole[P - 1:].view(torch.int16))
    # into a larger buffer: the first n copies are written, the rest keeps its bytes
    buf = torch.full((9, H, W, 8), 3.0, dtype=torch.bfloat16, device=DEV)
    out = hipops.occlude_batch(x, p, s, first=50, n=4, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf[:4].view(torch.int16), whole[50:54].view(torch.int16))
    assert bool((buf[4:] == 3.0).all())
    for first, n in ((P - 3, 4), (P, 1), (-1, 2), (0, 0)):        # first + n one beyond P, and friends
        with pytest.raises(PoseKernelError, match="copies"):
            hipops.occlude_batch(x, p, s, first=first, n=n)
    with pytest.raises(PoseKernelError, match="inside the destination"):
        hipops.occlude_batch(whole[3], p, s, out=whole)           # the source must not alias the destination
    with pytest.raises(PoseKernelError, match="extent - patch"):
        hipops.occlude_batch(_packed(12, 10), 12, 3)
    with pytest.raises(PoseKernelError, match="three floats"):
        hipops.occlude_batch(x, p, s, fill=(1.0, 2.0))


# ------------------------------------------------------------------------------------------------ pk_heatmap_summary
@functools.lru_cache(maxsize=None)
def _maps(lead, h, w):
    a = np.random.default_rng(h * 100 + w + len(lead)).standard_normal(lead + (h, w)).astype(np.float32)
    a.setflags(write=False)
    return a


# 1 x 1; 9 x 7 = 63 elements, fewer than the 256 threads; 20 x 15 = 300: the strided loop wraps with a ragged tail; 64 x 48 = 12 full rounds
@pytest.mark.parametrize("lead", [(1,), (3, 17)])
@pytest.mark.parametrize("hw", [(1, 1), (9, 7), (20, 15), (64, 48)])
def test_heatmap_summary_equals_the_restatement_bitwise_and_the_argmax_decoder(hw, lead):
    from infantposeestimation_gaussianbias_amd import hipops
    maps = _maps(lead, *hw)
    got = hipops.heatmap_summary(G(maps))
    assert tuple(got.shape) == lead + (4,) and got.dtype == F64
    got, want = got.cpu().numpy(), onp.summary(maps)
    assert np.array_equal(got, want)
    idx, mv, _ = hipops.argmax_decode(G(maps).reshape(1, -1, *hw), 0)
    assert np.array_equal(got[..., 1].reshape(-1), mv.cpu().numpy().reshape(-1).astype(np.float64))
    assert np.array_equal((got[..., 3] * hw[1] + got[..., 2]).reshape(-1), idx.cpu().numpy().reshape(-1).astype(np.float64))


def test_heatmap_summary_ties_constants_nan_and_types():
    from infantposeestimation_gaussianbias_amd import hipops
    m = np.array(_maps((5,), 20, 15))
    top = 8.0
    assert m.max() < top
    m[0, 7, 3] = m[0, 2, 11] = m[0, 19, 14] = top                 # equal maxima in three different threads and rounds: flat 41 wins
    m[1] = 0.25                                                   # constant: index 0
    m[2, 4, 4] = np.nan                                           # NaN: the sum is NaN, the maximum is not
    m[3] = -np.inf                                                # nothing above -inf
    m[4] = -np.abs(m[4])
    m[4, 6, 6], m[4, 9, 2] = -0.0, 0.0                            # -0 == +0: the first of them wins and is reported as it is stored
    got = hipops.heatmap_summary(G(m)).cpu().numpy()
    want = onp.summary(m)
    assert np.array_equal(got, want, equal_nan=True)
    assert got[0, 1:].tolist() == [top, 11.0, 2.0] and got[1].tolist() == [0.25 * 300, 0.25, 0.0, 0.0]
    assert np.isnan(got[2, 0]) and np.isfinite(got[2, 1]) and got[3].tolist() == [-np.inf, -np.inf, 0.0, 0.0]
    assert got[4, 1:].tolist() == [0.0, 6.0, 6.0] and np.signbit(got[4, 1])
    # bf16 is widened first; `out` may be a slice of a larger table
    h16 = G(m[:2]).to(torch.bfloat16)
    assert torch.equal(hipops.heatmap_summary(h16), hipops.heatmap_summary(h16.float()))
    table = torch.full((7, 4), -1.0, dtype=F64, device=DEV)
    back = hipops.heatmap_summary(G(m[:3]), out=table[2:5])
    assert back.data_ptr() == table[2:5].data_ptr() and np.array_equal(table[2:5].cpu().numpy(), want[:3], equal_nan=True)
    assert bool((table[:2] == -1).all()) and bool((table[5:] == -1).all())


def test_heatmap_summary_strides_over_more_maps_than_its_grid():
    """65 536 workgroups at most: with 3 maps more the first three workgroups take a second map each."""
    from infantposeestimation_gaussianbias_amd import hipops
    M = 65536 + 3
    maps = np.random.default_rng(9).standard_normal((M, 2, 3)).astype(np.float32)
    got = hipops.heatmap_summary(G(maps)).cpu().numpy()
    flat = maps.reshape(M, 6)
    idx = flat.argmax(1)
    assert np.array_equal(got[:, 1], flat.max(1).astype(np.float64)) and np.array_equal(got[:, 2], idx % 3) and np.array_equal(got[:, 3], idx // 3)
    seq = flat.astype(np.float64)                                 # six threads hold one element each: the butterfly's steps 4, 2, 1 add them
    want = ((seq[:, 0] + seq[:, 4]) + seq[:, 2]) + ((seq[:, 1] + seq[:, 5]) + seq[:, 3])
    for m in (0, 1, 2, 65535, 65536, 65537, M - 1):
        assert got[m, 0] == onp.fixed_order_sum(flat[m]) == want[m], m
    assert np.array_equal(got[:, 0], want)


# ------------------------------------------------------------------------------------------------ pk_occlusion_paint
@functools.lru_cache(maxsize=None)
def _table(P, K=3):
    g = np.random.default_rng(P)
    t = np.concatenate([g.standard_normal((P + 1, K, 2)) * 40, g.integers(0, 48, (P + 1, K, 2)).astype(np.float64)], -1)
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("measure", ["sum", "max", "shift"])
@pytest.mark.parametrize("shape", SHAPES)
def test_occlusion_paint_equals_the_literal_loop_bitwise(shape, measure):
    from infantposeestimation_gaussianbias_amd import hipops
    H, W, p, s = shape
    ny, nx = onp.grid(H, W, p, s)
    t = _table(ny * nx)
    base, table = t[0], t[1:]
    got = hipops.occlusion_paint(G(base, F64), G(table, F64), H, W, p, s, measure)
    assert tuple(got.shape) == (3, H, W) and got.dtype == F64
    want = onp.paint_loop(onp.values(base, table, measure), H, W, p, s)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.any() and not want[:, (ny - 1) * s + p:].any() and not want[:, :, (nx - 1) * s + p:].any()
    again = hipops.occlusion_paint(G(base, F64), G(table, F64).view(ny, nx, 3, 4), H, W, p, s, measure)      # the table in grid shape
    assert torch.equal(got, again)


def test_occlusion_paint_refuses_what_it_cannot_paint():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    t = _table(6)
    base, table = G(t[0], F64), G(t[1:], F64)
    hipops.occlusion_paint(base, table, 12, 10, 4, 3)
    with pytest.raises(PoseKernelError, match="positions"):
        hipops.occlusion_paint(base, table[:5], 12, 10, 4, 3)
    with pytest.raises(PoseKernelError, match="extent - patch"):
        hipops.occlusion_paint(base, table, 12, 10, 12, 3)
    with pytest.raises(PoseKernelError, match="measure"):
        hipops.occlusion_paint(base, table, 12, 10, 4, 3, "mean")


# ------------------------------------------------------------------------------------------------ model
@functools.lru_cache(maxsize=None)
def _model(name):
    import json
    import os
    from conftest import GOLDEN
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        keys = json.load(f)
    bb, head, spec, salt = {"hrnet_w18": ("hrnet_w18", "heatmap", "hrnet_w18_heatmap", 41),
                            "hrformer_small": ("hrformer_small", "fusion", "hrformer_small_fusion", 40)}[name]
    m = PoseEstimator(bb, 17, False, head, True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(keys[spec], salt).items()}, strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _single_forwards(name):
    """The reference's procedure on the model: the un-occluded forward, then one batch-1 forward per torch-made occluded clone, in the
    order of its loops; every map summarised by the restatement.  -> base (17,4), table (6,17,4)."""
    m, x = _model(name), G(synth_input("occlusion", (1, 3, 128, 96)))
    assert onp.grid(128, 96, 32, 32) == (3, 2)
    with torch.no_grad():
        base = onp.summary(m(x)["heatmaps"].float().cpu().numpy()[0])
        rows = []
        for i in range(0, 128 - 32, 32):
            for j in range(0, 96 - 32, 32):
                xo = x.clone()
                xo[:, :, i:i + 32, j:j + 32] = 0
                rows.append(onp.summary(m(xo)["heatmaps"].float().cpu().numpy()[0]))
    table = np.stack(rows)
    assert table.shape == (6, 17, 4) and all(not np.array_equal(r, base) for r in table)      # every patch changes something
    return base, table


@pytest.mark.parametrize("name", ["hrnet_w18", "hrformer_small"])
def test_sweep_in_chunks_equals_six_single_forwards_bitwise(name):
    from infantposeestimation_gaussianbias_amd import nnops, utils
    m, x = _model(name), G(synth_input("occlusion", (1, 3, 128, 96)))
    base, table = _single_forwards(name)
    res = utils.occlusion_sensitivity_maps(m, x, 32, 32, batch_size=4)          # chunks of 4 and 2
    assert res["grid"] == (3, 2) and tuple(res["table"].shape) == (3, 2, 17, 4) and tuple(res["base"].shape) == (17, 4)
    assert res["maps"].is_cuda and res["maps"].dtype == F64 and tuple(res["maps"].shape) == (17, 128, 96)
    assert np.array_equal(res["base"].cpu().numpy(), base)
    assert np.array_equal(res["table"].cpu().numpy().reshape(6, 17, 4), table)
    assert np.array_equal(res["maps"].cpu().numpy(), onp.paint_loop(onp.values(base, table, "sum"), 128, 96, 32, 32))
    for measure in ("max", "shift"):
        got = utils.occlusion_sensitivity_maps(m, x, 32, 32, measure=measure, batch_size=4)
        assert np.array_equal(got["maps"].cpu().numpy(), onp.paint_loop(onp.values(base, table, measure), 128, 96, 32, 32)), measure
        assert torch.equal(got["table"], res["table"])
    for other in (utils.occlusion_sensitivity_maps(m, x, 32, 32, batch_size=64),                   # one chunk of 6
                  utils.occlusion_sensitivity_maps(m, x[0], 32, 32, batch_size=1),                 # (3,H,W), six chunks of 1
                  utils.occlusion_sensitivity_maps(m, nnops.to_features(x), 32, 32, batch_size=5)):    # the packed image
        assert all(torch.equal(other[k], res[k]) for k in ("maps", "base", "table"))
    # a non-zero fill is the torch-made clone with that fill
    got = utils.occlusion_sensitivity_maps(m, x, 32, 32, fill=FILL, batch_size=4)
    xo = x.clone()
    xo[:, :, 64:96, 32:64] = G(np.array(FILL, np.float32))[None, :, None, None]
    with torch.no_grad():
        want = onp.summary(m(xo)["heatmaps"].float().cpu().numpy()[0])
    assert np.array_equal(got["table"][2, 1].cpu().numpy(), want) and not np.array_equal(want, table[5])


def test_analyzer_returns_the_map_of_one_joint_and_training_mode_raises():
    from infantposeestimation_gaussianbias_amd import utils
    m, x = _model("hrnet_w18"), G(synth_input("occlusion", (1, 3, 128, 96)))
    maps = utils.occlusion_sensitivity_maps(m, x, 32, 32)["maps"]
    one = utils.SensitivityAnalyzer.occlusion_sensitivity(m, x, target_keypoint=5, patch_size=32, stride=32)
    assert isinstance(one, np.ndarray) and one.dtype == np.float64 and one.shape == (128, 96)
    assert np.array_equal(one, maps[5].cpu().numpy()) and one.any()
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            utils.occlusion_sensitivity_maps(m, x, 32, 32)
    finally:
        m.eval()
    with pytest.raises(ValueError, match="one image"):
        utils.occlusion_sensitivity_maps(m, torch.cat([x, x]), 32, 32)
    with pytest.raises(RuntimeError, match="extent - patch"):
        utils.occlusion_sensitivity_maps(m, x, 128, 32)


# ------------------------------------------------------------------------------------------------ surface
@functools.lru_cache(maxsize=None)
def _pose():
    import inference
    torch.manual_seed(11)
    return inference.PoseInference(config="hrnet_w18", flip_test=False)


def test_pose_inference_sweeps_the_crop_of_predict():
    from infantposeestimation_gaussianbias_amd import utils
    pose = _pose()
    img = np.random.default_rng(12).integers(0, 256, (120, 160, 3)).astype(np.uint8)
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    res = pose.occlusion_sensitivity(img, bbox, patch_size=32, stride=32)
    x, c, s = pose.preprocess(img, bbox)
    want = utils.occlusion_sensitivity_maps(pose.model, x, 32, 32)
    w, h = pose.input_size
    assert res["grid"] == want["grid"] == onp.grid(h, w, 32, 32) == (3, 2) and tuple(res["maps"].shape) == (17, h, w)
    assert all(torch.equal(res[k], want[k]) for k in ("maps", "base", "table")) and bool(res["maps"].any())
    assert np.array_equal(res["center"], c) and np.array_equal(res["scale"], s)
    some = pose.occlusion_sensitivity(img, bbox, joints=[5, 2], patch_size=32, stride=32, measure="max")
    wmax = utils.occlusion_sensitivity_maps(pose.model, x, 32, 32, measure="max")
    assert torch.equal(some["maps"], wmax["maps"][[5, 2]]) and torch.equal(some["base"], wmax["base"][[5, 2]])
    assert torch.equal(some["table"], wmax["table"][:, :, [5, 2]])


def test_occlusion_map_switch_draws_the_joint_where_the_crop_lies(tmp_path, capsys):
    import inference
    from PIL import Image
    pose = _pose()
    img = np.random.default_rng(12).integers(0, 256, (120, 160, 3)).astype(np.uint8)
    bbox = np.array([60.0, 30.0, 120.0, 100.0])
    out = tmp_path / "occlusion.png"
    args = argparse.Namespace(occlusion_map=5, occlusion_patch=32, occlusion_stride=32, occlusion_measure="sum", output=str(out))
    res = inference.main_occlusion(args, pose, img, bbox)
    text = capsys.readouterr().out
    assert "3 x 2 = 6 patches" in text and "largest drop for joint 5" in text
    drop = (res["base"][5, 0] - res["table"][:, :, 5, 0]).cpu().numpy()
    a, b = np.unravel_index(np.argmax(drop), drop.shape)
    assert f"crop rows {a * 32} .. {a * 32 + 31}, columns {b * 32} .. {b * 32 + 31}" in text
    drawn = np.asarray(Image.open(out).convert("RGB"))[:, :, ::-1]
    assert drawn.shape == img.shape
    changed = (drawn != img).any(-1)
    assert changed.any() and not changed[:, :10].any() and not changed[:5].any()      # only where the crop lies
    with pytest.raises(SystemExit):
        inference.main_occlusion(argparse.Namespace(**{**vars(args), "occlusion_map": 17}), pose, img, bbox)
