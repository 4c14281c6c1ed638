"""Online hard keypoint mining without a GPU: the float64 restatement (tests/ohkm_np.py) against the textbook torch form and autograd on
the CPU, the margin condition of every random case the GPU tests use, the two entries in the header and their refusals, the legacy-yaml
mapping, the constructors' validation, and train.py's flags.  The kernels themselves need a device: nothing here gets past their
argument checks."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import ohkm_np as onp
from conftest import GOLDEN

ALL_CASES = [(shape, weighted, seed) for shape in onp.SHAPES for weighted in (True, False) for seed in onp.case_seeds(shape, weighted)]


def _textbook(pred, target, weight, topk, scale):
    """topk over ((w (p - t))^2).mean((2, 3)), gather, sum / topk, mean -- HRNet's JointsOHKMMSELoss / mmpose's KeypointOHKMMSELoss in
    float64 torch; -> loss, per_map, grad of the loss with respect to pred."""
    p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
    t = torch.from_numpy(np.asarray(target, np.float64))
    B, K = p.shape[:2]
    w = torch.ones(B, K, dtype=torch.float64) if weight is None else torch.from_numpy(np.asarray(weight, np.float64))
    per_map = ((w[:, :, None, None] * (p - t)) ** 2).mean((2, 3))
    idx = torch.topk(per_map, topk, dim=1, sorted=False).indices
    loss = scale * (torch.gather(per_map, 1, idx).sum(1) / topk).mean()
    loss.backward()
    return float(loss.detach()), per_map.detach().numpy(), idx.numpy(), p.grad.numpy()


@pytest.mark.parametrize("shape,weighted,seed", ALL_CASES)
def test_restatement_equals_the_textbook_form_and_autograd(shape, weighted, seed):
    B, K, H, W, topk = shape
    pred, target, weight = onp.cases(seed, B, K, H, W)
    weight = weight if weighted else None
    for scale in (1.0, 0.5):
        loss, per_map, mask, grad = onp.ohkm_np(pred, target, weight, topk, scale)
        tl, tpm, idx, tg = _textbook(pred, target, weight, topk, scale)
        assert np.abs(per_map - tpm).max() <= 64 * 2.0 ** -52 * tpm.max()          # float64 sums in another order
        assert abs(loss - tl) <= 64 * 2.0 ** -52 * abs(tl)
        # torch's selection: the same set wherever the boundary is not a tie of exact zeros (there any of the zero maps serves: they add 0)
        want = np.zeros((B, K), np.uint8)
        np.put_along_axis(want, idx, 1, 1)
        assert mask.sum(1).tolist() == [topk] * B
        differ = (want != mask)
        assert not (differ & (per_map != 0)).any()
        # gradients: compare where both select; a zero-weight map's gradient is zero whether it is selected or not
        assert np.abs(grad - tg).max() <= 64 * 2.0 ** -52 * np.abs(tg).max()
        assert not grad[mask == 0].any()
    g3 = onp.ohkm_np(pred, target, weight, topk, 1.0, grad_out=3.0)[3]
    assert np.abs(g3 - 3.0 * grad * 2.0).max() <= 4 * 2.0 ** -52 * np.abs(g3).max()          # `grad` is scale 0.5's: linear in both


def test_margin_condition_holds_for_every_random_case():
    """In float64, the topk-th and (topk+1)-th largest error of every sample differ by at least 16 (HW + 4) 2^-24 relative (exact zeros
    excepted): 16 times the worst-case fp32 summation error, so fp32 rounding cannot change a selection.  With the weights, seeds 0, 1, 2
    of every shape satisfy it; the smallest gap there is about 4 times the requirement (70 times the error)."""
    smallest = math.inf
    for shape in onp.SHAPES:
        assert onp.case_seeds(shape, True) == (0, 1, 2), shape
    for shape, weighted, seed in ALL_CASES:
        B, K, H, W, topk = shape
        pred, target, weight = onp.cases(seed, B, K, H, W)
        gap = onp.margin(onp.ohkm_np(pred, target, weight if weighted else None, topk, 1.0)[1], topk)
        print(shape, "weighted" if weighted else "plain", seed, f"gap / required = {gap / onp.required_margin(H * W):.2f}")
        assert gap >= onp.required_margin(H * W), (shape, weighted, seed)
        if weighted:
            smallest = min(smallest, gap / onp.required_margin(H * W))
    assert 4.0 <= smallest < 5.0, smallest


def test_ranking_is_torch_topk_order_with_nans_and_ties():
    row = np.array([1.0, np.nan, 3.0, 3.0, 0.0, np.nan, 0.0, 2.0])
    assert onp.rank_order(row) == [1, 5, 2, 3, 7, 0, 4, 6]
    pred = np.zeros((1, 8, 2, 2), np.float32)
    pred[0, :, 0, 0] = np.nan_to_num(row, nan=0.0) ** 0.5 * 2          # per_map = row where it is a number
    pred[0, 1, 1, 1] = pred[0, 5, 0, 1] = np.nan
    loss, per_map, mask, _ = onp.ohkm_np(pred, np.zeros_like(pred), None, 3, 1.0)
    assert np.isnan(loss) and mask[0].tolist() == [0, 1, 1, 0, 0, 1, 0, 0]
    assert np.allclose(per_map[0, [0, 2, 3, 4, 6, 7]], row[[0, 2, 3, 4, 6, 7]])


def test_exact_case_ties_fall_to_the_lower_index():
    pred, target, weight, topk = onp.exact_case()
    loss, per_map, mask, _ = onp.ohkm_np(pred, target, weight, topk, 1.0)
    assert np.abs(pred - target).max() <= 4 and not ((pred - target) % 0.5).any() and set(np.unique(weight)) == {0.0, 1.0}
    assert np.array_equal(per_map, per_map.astype(np.float32)) and loss == float(np.float32(loss))        # exact in float32 too
    assert per_map[0, 1] == per_map[0, 3] == per_map[0, 4] == per_map[0, 6]
    assert mask.tolist() == [[0, 1, 1, 1, 0, 0, 0, 1], [1, 0, 0, 1, 0, 1, 0, 1], [1, 1, 1, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 1, 1, 1]]


# ------------------------------------------------------------------------------------------------ C-ABI
def test_both_entries_are_declared_exported_and_refuse_bad_arguments_before_any_launch():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_ohkm_loss_fwd", 13), ("pk_ohkm_loss_bwd", 12)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(_lib.lib, name)
    L, p = _lib.lib, 64                           # a non-null pointer value that is never dereferenced: the checks refuse first

    def fwd(pred=p, target=p, per_map=p, mask=p, loss=p, B=2, K=17, HW=35, topk=8, scale=1.0):
        return L.pk_ohkm_loss_fwd(pred, target, None, per_map, mask, loss, None, B, K, HW, topk, scale, None)

    def bwd(pred=p, target=p, mask=p, d_pred=p, B=2, K=17, HW=35, topk=8, scale=1.0):
        return L.pk_ohkm_loss_bwd(pred, target, None, mask, None, d_pred, B, K, HW, topk, scale, None)

    for fn, name in ((fwd, b"pk_ohkm_loss_fwd"), (bwd, b"pk_ohkm_loss_bwd")):
        for kw, word in (({"topk": 0}, b"topk=0"), ({"topk": 18}, b"topk=18"), ({"K": 257, "topk": 8}, b"K=257"), ({"K": 0}, b"K=0"),
                         ({"B": 0}, b"B=0"), ({"HW": 0}, b"HW=0"), ({"B": -1}, b"B=-1"), ({"scale": 0.0}, b"scale=0"),
                         ({"scale": -1.0}, b"scale=-1"), ({"scale": math.inf}, b"scale=inf"), ({"scale": math.nan}, b"scale=nan"),
                         ({"pred": None}, b"null pointer"), ({"target": None}, b"null pointer"), ({"mask": None}, b"null pointer")):
            assert fn(**kw) == -1, (name, kw)
            msg = L.pk_last_error_string()
            assert name in msg and word in msg, (msg, kw)
    for kw in ({"per_map": None}, {"loss": None}):
        assert fwd(**kw) == -1 and b"pk_ohkm_loss_fwd: null pointer" in L.pk_last_error_string()
    assert bwd(d_pred=None) == -1 and b"pk_ohkm_loss_bwd: null pointer" in L.pk_last_error_string()


def test_op_refuses_host_tensors_and_bad_shapes_without_a_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    z = torch.zeros
    with pytest.raises(PoseKernelError, match="no CPU implementation"):
        hipops.ohkm_loss(z(2, 17, 5, 7), z(2, 17, 5, 7), z(2, 17), 8)
    with pytest.raises(PoseKernelError, match="no CPU implementation"):
        hipops.ohkm_loss(z(2, 17, 5, 7), z(2, 17, 5, 7), None, 8, scale=0.5, counts=z(17, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ configuration
def test_yaml_mapping_and_config_defaults(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.configs.config import ModelConfig
    fields = [f.name for f in dataclasses.fields(ModelConfig)]
    assert "ohkm_topk" not in fields and "ohkm_weight" not in fields and (ModelConfig.ohkm_topk, ModelConfig.ohkm_weight) == (0, 1.0)
    for src in (None, "hrformer_small", "hrnet_w18", os.path.join(GOLDEN, "eval_blocks_preemie_optimized.yaml"),
                os.path.join(GOLDEN, "eval_blocks_default.yaml")):
        cfg = get_config(src)
        assert cfg.model.ohkm_topk == 0 and cfg.model.ohkm_weight == 1.0, src

    def y(text):
        p = tmp_path / "legacy.yaml"
        p.write_text(text)
        return get_config(str(p)).model

    m = y("LOSS:\n  USE_OHKM: true\n")
    assert (m.ohkm_topk, m.ohkm_weight) == (8, 1.0)                       # HRNet's default TOPK
    m = y("LOSS:\n  USE_OHKM: true\n  TOPK: 5\n  OHKM_WEIGHT: 0.25\n")
    assert (m.ohkm_topk, m.ohkm_weight) == (5, 0.25)
    m = y("LOSS:\n  USE_OHKM: false\n  TOPK: 5\n  OHKM_WEIGHT: 0.25\n")
    assert (m.ohkm_topk, m.ohkm_weight) == (0, 1.0)
    m = y("LOSS:\n  MORPH_WEIGHT: 0.15\n  MORPH_LAMBDA: 1.2\n  TOPK: 5\n")      # a block without USE_OHKM
    assert m.ohkm_topk == 0
    m = y("MODEL:\n  NUM_JOINTS: 13\nLOSS:\n  USE_OHKM: true\n  TOPK: 13\n")
    assert m.ohkm_topk == 13
    with pytest.raises(ValueError, match="LOSS.TOPK"):
        y("MODEL:\n  NUM_JOINTS: 13\nLOSS:\n  USE_OHKM: true\n  TOPK: 14\n")
    with pytest.raises(ValueError, match="LOSS.TOPK"):
        y("LOSS:\n  USE_OHKM: true\n  TOPK: 0\n")
    with pytest.raises(ValueError, match="LOSS.OHKM_WEIGHT"):
        y("LOSS:\n  USE_OHKM: true\n  OHKM_WEIGHT: -1\n")
    assert (ModelConfig.ohkm_topk, get_config().model.ohkm_topk) == (0, 0)       # a loaded yaml does not leak into the class


def test_constructors_reject_bad_topk_and_weight():
    from infantposeestimation_gaussianbias_amd.models import FusionPoseLoss, KeypointMSELoss, PoseEstimator
    from infantposeestimation_gaussianbias_amd.models.losses import JointsOHKMMSELoss
    from infantposeestimation_gaussianbias_amd.models.pose_estimator import build_model
    from infantposeestimation_gaussianbias_amd.configs import get_config
    for bad in (-1, 257, 2.5, "8", True, None):
        with pytest.raises(ValueError, match="ohkm_topk"):
            KeypointMSELoss(True, ohkm_topk=bad)
        with pytest.raises(ValueError, match="ohkm_topk"):
            FusionPoseLoss(ohkm_topk=bad)
        with pytest.raises(ValueError, match="topk"):
            JointsOHKMMSELoss(True, topk=bad)
    with pytest.raises(ValueError, match="topk"):
        JointsOHKMMSELoss(True, topk=0)                       # this class has no "off"
    for bad in (-0.5, math.inf, math.nan, "1", None):
        with pytest.raises(ValueError, match="ohkm_weight"):
            FusionPoseLoss(ohkm_topk=8, ohkm_weight=bad)
    for kw in ({"ohkm_topk": 18}, {"ohkm_topk": -1}, {"ohkm_topk": 8, "ohkm_weight": -1.0}, {"ohkm_topk": 8, "ohkm_weight": math.nan}):
        with pytest.raises(ValueError, match="ohkm"):
            PoseEstimator("hrnet_w18", 17, False, "heatmap", **kw)
    with pytest.raises(ValueError, match="ohkm_topk"):
        KeypointMSELoss(True, ohkm_topk=14, num_keypoints=13)
    cfg = get_config("hrnet_w18")
    cfg.model.pretrained, cfg.model.ohkm_topk = False, 18
    with pytest.raises(ValueError, match="ohkm_topk"):
        build_model(cfg)
    # the reference's positional signature still holds, the new arguments come after it, and the defaults are "off"
    fl = FusionPoseLoss(1.0, 1.0, 0.5, 0.1, 0.05, 0.05, 2.0, True)
    assert fl.ohkm_topk == 0 and fl.selection_counts() is None and KeypointMSELoss(True).ohkm_topk == 0
    fl = FusionPoseLoss(1.0, 1.0, 0.5, 0.1, 0.05, 0.05, 2.0, True, 8, 0.5, 17)
    assert (fl.ohkm_topk, fl.ohkm_weight) == (8, 0.5) and fl.selection_counts().tolist() == [0] * 17
    assert "_ohkm_counts" not in fl.state_dict() and JointsOHKMMSELoss().topk == 8
    cfg.model.ohkm_topk, cfg.model.ohkm_weight = 8, 0.5
    m = build_model(cfg)
    assert (m.ohkm_topk, m.ohkm_weight, m.loss_fn.ohkm_topk) == (8, 0.5, 8) and m.selection_counts().tolist() == [0] * 17


def test_padded_twin_builder_passes_the_settings_on():
    """hrnet_w18 and hrformer_base run as their 8-aligned twins: a setting that stopped at the real model would silently do nothing."""
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    from infantposeestimation_gaussianbias_amd.models.padded import _build_twin
    real = PoseEstimator("hrnet_w18", 17, False, "heatmap", ohkm_topk=8, ohkm_weight=0.5)
    twin = _build_twin(real)
    assert (twin.ohkm_topk, twin.ohkm_weight, twin.loss_fn.ohkm_topk) == (8, 0.5, 8)
    assert _build_twin(PoseEstimator("hrnet_w18", 17, False, "heatmap")).loss_fn.ohkm_topk == 0


def test_train_parser_accepts_the_flags():
    import train
    args = train.build_parser().parse_args(["--ohkm", "8", "--ohkm_weight", "0.5"])
    assert (args.ohkm, args.ohkm_weight) == (8, 0.5)
    args = train.build_parser().parse_args([])
    assert args.ohkm is None and args.ohkm_weight is None

    class _Model:
        def selection_counts(self, reset=False):
            return np.array([1, 0, 3], np.int64)

    assert train.selection_report(_Model(), ["a", "b", "c"]) == "c 75.0%, a 25.0%, b 0.0%"
