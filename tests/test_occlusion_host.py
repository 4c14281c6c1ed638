"""Occlusion sensitivity without a GPU: the four entries in the header, the grid count against the reference's loop bounds, every refusal
with its text, the restatement's closed form against its literal loop, the restatement's summary order, and the switches of inference.py.
The kernels themselves raise without a device, so nothing here calls them past their argument checks."""
import numpy as np
import pytest
import torch

import occlusion_np as onp

BAD = [(0, 4, 2), (8, 0, 2), (8, 4, 0), (-3, 4, 2), (8, -1, 2), (8, 4, -5)]


def _err():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib.lib.pk_last_error_string().decode()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_four_entries_are_declared_with_their_argument_counts():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name, n_args in (("pk_occlusion_positions", 3), ("pk_occlude_batch", 10), ("pk_heatmap_summary", 6), ("pk_occlusion_paint", 10)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(_lib.lib, name), name


def test_positions_agree_with_the_loop_bounds_of_the_reference():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    L = _lib.lib
    assert len(onp.GRID_CASES) == 8
    for H, W, p, s in onp.GRID_CASES:
        for e in (H, W):
            want = len(range(0, e - p, s))
            assert L.pk_occlusion_positions(e, p, s) == want == onp.count(e, p, s) == hipops.occlusion_positions(e, p, s), (e, p, s)
    assert onp.grid(256, 192, 16, 8) == (30, 22) and onp.grid(16, 16, 16, 8) == (0, 0)
    assert onp.positions(256, 16, 8)[-1] == 232 and onp.positions(192, 16, 8)[-1] == 168      # 240 and 176, i.e. extent - patch, are not taken
    for e in range(1, 40):                                        # and every small case
        for p in range(1, 12):
            for s in range(1, 12):
                assert L.pk_occlusion_positions(e, p, s) == len(range(0, e - p, s)), (e, p, s)
    assert L.pk_occlusion_positions(2 ** 31 - 1, 1, 2 ** 31 - 1) == 1 and L.pk_occlusion_positions(2 ** 31 - 1, 1, 1) == 2 ** 31 - 2


def test_positions_refuse_bad_arguments_with_text():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    for e, p, s in BAD:
        assert _lib.lib.pk_occlusion_positions(e, p, s) == -1
        assert _err() == f"pk_occlusion_positions: bad argument extent={e} patch={p} stride={s} (each at least 1)"
        with pytest.raises(_lib.PoseKernelError, match="each at least 1"):
            hipops.occlusion_positions(e, p, s)
    with pytest.raises(_lib.PoseKernelError, match=r"range\(0, extent - patch, stride\)"):
        hipops.occlusion_grid(16, 16, 16, 8)


def test_every_refusal_of_the_three_launching_entries_comes_back_with_its_text():
    from infantposeestimation_gaussianbias_amd import _lib
    L, p = _lib.lib, 4096                                         # a non-null aligned pointer value that is never dereferenced: the checks refuse first
    far = p + (1 << 30)
    rule = "no patch position: rows and columns start at range(0, extent - patch, stride), which is empty"

    def occlude(x=p, out=far, H=33, W=25, patch=7, stride=3, first=0, n=4):
        return L.pk_occlude_batch(x, out, H, W, patch, stride, first, n, None, None)

    ny, nx = onp.grid(33, 25, 7, 3)
    assert (ny, nx) == (9, 6)
    assert occlude(x=None) == -1 and _err() == "pk_occlude_batch: null pointer"
    assert occlude(out=None) == -1 and _err() == "pk_occlude_batch: null pointer"
    assert occlude(H=7) == -1 and _err() == f"pk_occlude_batch: {rule} for H=7 W=25 patch=7"
    assert occlude(W=5) == -1 and _err() == f"pk_occlude_batch: {rule} for H=33 W=5 patch=7"
    assert occlude(stride=0) == -1 and _err() == "pk_occlude_batch: bad argument H=33 W=25 patch=7 stride=0 (each at least 1)"
    assert occlude(first=-1) == -1 and _err() == "pk_occlude_batch: copies -1 .. 2 of 54 (9 x 6 positions)"
    assert occlude(n=0) == -1
    assert occlude(first=51, n=4) == -1 and _err() == "pk_occlude_batch: copies 51 .. 54 of 54 (9 x 6 positions)"
    assert occlude(H=40000, W=40000, patch=1, stride=1, n=3) == -1
    assert _err() == "pk_occlude_batch: 3 copies of 40000 x 40000 pixels overflow 32-bit pixel indices"
    # the source inside, at the end of and just before the destination; side by side is fine but cannot be launched here
    size = 33 * 25 * 16
    for x in (far, far + 4 * size - 16, far - size + 16):
        assert occlude(x=x) == -1 and _err() == "pk_occlude_batch: the source image lies inside the destination", x
    assert occlude(x=p + 8) == -1 and _err() == "pk_occlude_batch: pointers must be 16-byte aligned"

    def summary(hm=p, out=p, M=3, h=9, w=7):
        return L.pk_heatmap_summary(hm, out, M, h, w, None)

    assert summary(hm=None) == -1 and _err() == "pk_heatmap_summary: null pointer"
    assert summary(out=None) == -1 and _err() == "pk_heatmap_summary: null pointer"
    assert summary(M=0) == -1 and _err() == "pk_heatmap_summary: bad shape M=0 h=9 w=7"
    assert summary(h=0) == -1 and summary(w=-1) == -1
    assert summary(h=65536, w=32768) == -1 and _err() == "pk_heatmap_summary: bad shape M=3 h=65536 w=32768"

    def paint(base=p, table=p, maps=p, measure=0, K=3, H=33, W=25, patch=7, stride=3):
        return L.pk_occlusion_paint(base, table, maps, measure, K, H, W, patch, stride, None)

    for name in ("base", "table", "maps"):
        assert paint(**{name: None}) == -1 and _err() == "pk_occlusion_paint: null pointer", name
    assert paint(measure=3) == -1 and _err() == "pk_occlusion_paint: measure 3 (0 sum, 1 max, 2 shift)"
    assert paint(measure=-1) == -1
    assert paint(K=0) == -1 and _err() == "pk_occlusion_paint: bad joint count K=0"
    assert paint(H=16, W=16, patch=16, stride=8) == -1 and _err() == f"pk_occlusion_paint: {rule} for H=16 W=16 patch=16"
    assert paint(patch=0) == -1 and _err() == "pk_occlusion_paint: bad argument H=33 W=25 patch=0 stride=3 (each at least 1)"
    assert paint(K=17, H=40000, W=40000) == -1 and _err() == "pk_occlusion_paint: 17 maps of 40000 x 40000 pixels overflow 32-bit indices"


def test_op_layer_refuses_before_any_launch(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    assert hipops.OCCLUSION_MEASURES == onp.MEASURES
    z = torch.zeros
    with pytest.raises(PoseKernelError):                          # host tensors: no CPU implementation
        hipops.occlude_batch(z(12, 10, 8, dtype=torch.bfloat16), 4, 3)
    with pytest.raises(PoseKernelError):
        hipops.heatmap_summary(z(3, 9, 7))
    with pytest.raises(PoseKernelError):
        hipops.occlusion_paint(z(3, 4, dtype=torch.float64), z(6, 3, 4, dtype=torch.float64), 12, 10, 4, 3)
    with pytest.raises(PoseKernelError, match="measure"):
        hipops.occlusion_paint(z(3, 4, dtype=torch.float64), z(6, 3, 4, dtype=torch.float64), 12, 10, 4, 3, "mean")
    with pytest.raises(PoseKernelError, match="extent - patch"):
        hipops.occlusion_paint(z(3, 4, dtype=torch.float64), z(6, 3, 4, dtype=torch.float64), 16, 16, 16, 8)


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("case", onp.GRID_CASES)
def test_closed_form_equals_the_literal_loop(case):
    H, W, p, s = case
    ny, nx = onp.grid(H, W, p, s)
    vals = np.random.default_rng(H * 1000 + W).standard_normal((ny * nx, 3))
    loop, closed = onp.paint_loop(vals, H, W, p, s), onp.paint_closed(vals, H, W, p, s)
    assert loop.shape == (3, H, W) and np.array_equal(loop, closed)
    if ny * nx == 0:
        assert not loop.any()
    else:
        assert np.array_equal(loop[:, 0, 0], vals[0]) and np.array_equal(loop[:, (ny - 1) * s + p - 1, (nx - 1) * s + p - 1], vals[-1])
        assert not loop[:, (ny - 1) * s + p:].any() and not loop[:, :, (nx - 1) * s + p:].any()       # the margins stay 0
        if s > p:
            assert not loop[:, p:s].any() and not loop[:, :, p:s].any()                                 # and so do the gaps
    if case == (256, 192, 16, 8):
        assert not loop[:, 248:].any() and not loop[:, :, 184:].any() and loop[:, 247, 183].all()


def test_summary_order_is_a_sum_and_the_first_maximum_wins():
    g = np.random.default_rng(3)
    for n in (1, 63, 255, 256, 257, 300, 3072):
        row = g.standard_normal(n).astype(np.float32)
        want = float(np.sum(row.astype(np.float64)))
        assert abs(onp.fixed_order_sum(row) - want) <= (n + 16) * 2.0 ** -52 * float(np.abs(row.astype(np.float64)).sum())
    assert onp.fixed_order_sum(np.arange(1000, dtype=np.float32)) == 499500.0          # exact in any order
    m = np.zeros((4, 5), np.float32)
    m[1, 2] = m[3, 0] = 2.0
    assert onp.summary(m).tolist() == [4.0, 2.0, 2.0, 1.0]
    m[0, 3] = np.nan
    s = onp.summary(m)
    assert np.isnan(s[0]) and s[1:].tolist() == [2.0, 2.0, 1.0]
    assert onp.summary(np.full((2, 2), -np.inf, np.float32))[1:].tolist() == [-np.inf, 0.0, 0.0]
    assert onp.summary(np.full((3, 2, 2), 0.5, np.float32)).tolist() == [[2.0, 0.5, 0.0, 0.0]] * 3


def test_occluded_copies_follow_the_loop_order():
    chw = np.random.default_rng(5).standard_normal((3, 12, 10)).astype(np.float32)
    packed = onp.pack_image(chw)
    assert not packed[..., 3:].any() and onp.bf16_bits(np.float32(1.0)) == 0x3f80 and onp.bf16_bits(np.float32(1.00390625)) == 0x3f80
    assert onp.bf16_bits(np.float32(1.01171875)) == 0x3f82                                # a tie goes to the even neighbour
    copies = onp.occluded_copies(packed, 4, 3, fill=(0.5, -1.0, 2.0))
    assert copies.shape == (3 * 2, 12, 10, 8)
    c = copies[1 * 2 + 1]                                          # a = 1, b = 1: rows 3..6, columns 3..6
    assert (c[3:7, 3:7] == np.array([0x3f00, 0xbf80, 0x4000, 0, 0, 0, 0, 0], np.uint16)).all()
    c = c.copy()
    c[3:7, 3:7] = packed[3:7, 3:7]
    assert np.array_equal(c, packed)


# ------------------------------------------------------------------------------------------------ the public surface
def test_the_module_is_exported_and_has_no_host_path():
    from infantposeestimation_gaussianbias_amd import utils
    assert {"sensitivity", "SensitivityAnalyzer", "occlusion_sensitivity_maps"} <= set(utils.__all__)
    assert utils.SensitivityAnalyzer.occlusion_sensitivity is not None and callable(utils.occlusion_sensitivity_maps)
    model = torch.nn.Linear(1, 1).eval()
    with pytest.raises(TypeError, match="device tensor"):
        utils.occlusion_sensitivity_maps(model, torch.zeros(1, 3, 32, 24))
    with pytest.raises(RuntimeError, match="eval"):
        utils.occlusion_sensitivity_maps(model.train(), torch.zeros(1, 3, 32, 24))
    with pytest.raises(ValueError, match="measure"):
        utils.occlusion_sensitivity_maps(model.eval(), torch.zeros(1, 3, 32, 24), measure="mean")


def test_inference_parser_accepts_the_occlusion_switches():
    import inference
    p = inference.build_parser()
    args = p.parse_args(["--input", "x.png"])
    assert args.occlusion_map is None and (args.occlusion_patch, args.occlusion_stride, args.occlusion_measure) == (16, 8, "sum")
    args = p.parse_args(["--input", "x.png", "--output", "y.png", "--occlusion_map", "5", "--occlusion_patch", "32", "--occlusion_stride", "16",
                         "--occlusion_measure", "shift"])
    assert (args.occlusion_map, args.occlusion_patch, args.occlusion_stride, args.occlusion_measure) == (5, 32, 16, "shift")
    with pytest.raises(SystemExit):
        p.parse_args(["--input", "x.png", "--occlusion_map", "5", "--occlusion_measure", "mean"])
    assert "clamped at 0" in p.format_help() and hasattr(inference.PoseInference, "occlusion_sensitivity")
