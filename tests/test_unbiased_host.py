"""Unbiased (DARK) decode, host side: the C-ABI prototype and its argument checks (made before any launch), the smoothing taps, the
legacy-yaml and command-line surface, and what the numpy restatement of the specification (tests/unbiased_np.py) says about accuracy,
about how often the step is taken and about its conditioning in float32.  Nothing here launches a kernel."""
import ctypes
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

import unbiased_np as unp


# ------------------------------------------------------------------------------------------------ C-ABI
def test_header_prototype_matches_the_library_symbol():
    from infantposeestimation_gaussianbias_amd import _lib
    ret, args = _lib.declared_symbols()["pk_unbiased_decode"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert ret == "int" and args == [P, P, I, P, P, P, P, I, I, I, P]
    fn = _lib.lib.pk_unbiased_decode
    assert fn.argtypes == args and fn.restype is ctypes.c_int


def test_entry_refuses_bad_arguments_before_any_launch():
    from infantposeestimation_gaussianbias_amd import _lib
    L = _lib.lib
    g = np.ones(32, np.float32)
    one, taps = 16, g.ctypes.data                  # any non-null address: the checks run before anything is touched
    cases = [((None, taps, 11, None, None, one, None, 1, 8, 8, None), b"null"),
             ((one, taps, 11, None, None, None, None, 1, 8, 8, None), b"null"),
             ((one, None, 11, None, None, one, None, 1, 8, 8, None), b"null")]
    for k in (10, 4, 1, 2, 0, -3, 33, 32):
        cases.append(((one, taps, k, None, None, one, None, 1, 8, 8, None), f"ksize {k}".encode()))
    for BK, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 32768)):
        cases.append(((one, taps, 11, None, None, one, None, BK, H, W, None), b"shape"))
    for args, word in cases:
        assert L.pk_unbiased_decode(*args) == -1 and word in L.pk_last_error_string(), (args, L.pk_last_error_string())


def test_op_layer_refuses_bad_arguments():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    hm = torch.zeros(1, 2, 8, 8)
    for k in (10, 1, 33, 0, 5.5, -3):
        with pytest.raises(_lib.PoseKernelError, match="kernel"):
            hipops.unbiased_decode(hm, k)
    with pytest.raises(_lib.PoseKernelError, match="HIP"):
        hipops.unbiased_decode(hm, 11)               # a host tensor: there is no CPU implementation


# ------------------------------------------------------------------------------------------------ taps
@pytest.mark.parametrize("k", [3, 5, 11, 17])
def test_taps_are_the_formula(k):
    from infantposeestimation_gaussianbias_amd import hipops
    g = hipops.unbiased_taps(k)
    assert g.dtype == np.float32 and g.shape == (k,) and hipops.unbiased_taps(k) is g            # cached per size
    assert np.array_equal(g, g[::-1])
    # k values rounded to float32 (each within 2^-24 relative of its float64 value, and those sum to 1), added in float64
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 2.0 ** -24 + 1e-15
    assert np.array_equal(g, unp.taps(k))
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    w = np.exp(-(np.arange(k) - (k - 1) / 2) ** 2 / (2 * sigma ** 2))
    assert np.array_equal(g, (w / w.sum()).astype(np.float32))
    if k == 3:      # sigma 0.8: not OpenCV's fixed (0.25, 0.5, 0.25) table
        assert sigma == 0.8 and abs(float(g[1]) - 1 / (1 + 2 * np.exp(-1 / 1.28))) < 1e-7 and g[1] != 0.5


# ------------------------------------------------------------------------------------------------ configuration
def _yaml(tmp_path, text):
    p = tmp_path / "legacy.yaml"
    p.write_text("MODEL:\n  NUM_JOINTS: 13\n" + text)
    return str(p)


def test_yaml_mapping_onto_decode(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import Config, get_config
    cfg = get_config()
    assert cfg.decode is None and cfg.modulate_kernel == 11
    assert not {"decode", "modulate_kernel"} & {f.name for f in dataclasses.fields(Config)}
    cfg = get_config(_yaml(tmp_path, "TEST:\n  DECODE: 'unbiased'\n  MODULATE_KERNEL: 17\n"))
    assert cfg.decode == "unbiased" and cfg.modulate_kernel == 17 and cfg.data.num_keypoints == 13
    cfg = get_config(_yaml(tmp_path, "TEST:\n  DECODE: shift\n"))
    assert cfg.decode == "shift" and cfg.modulate_kernel == 11
    cfg = get_config(_yaml(tmp_path, "TEST:\n  MODULATE_KERNEL: 5\n"))
    assert cfg.decode is None and cfg.modulate_kernel == 5
    # the keys both shipped yamls set true are not mapped: such a configuration decodes as it does today
    cfg = get_config(_yaml(tmp_path, "TEST:\n  POST_PROCESS: true\n  SHIFT_HEATMAP: true\n  FLIP_TEST: true\n"))
    assert cfg.decode is None and cfg.modulate_kernel == 11
    assert get_config(_yaml(tmp_path, "")).decode is None
    assert Config.decode is None and Config.modulate_kernel == 11          # a loaded yaml does not leak into the class
    for bad, key in (("DECODE: dark", "TEST.DECODE"), ("DECODE: true", "TEST.DECODE"), ("DECODE: 1", "TEST.DECODE"),
                     ("DECODE: unbiased\n  MODULATE_KERNEL: 10", "TEST.MODULATE_KERNEL"), ("MODULATE_KERNEL: 33", "TEST.MODULATE_KERNEL"),
                     ("MODULATE_KERNEL: 1", "TEST.MODULATE_KERNEL"), ("MODULATE_KERNEL: 5.5", "TEST.MODULATE_KERNEL"),
                     ("MODULATE_KERNEL: eleven", "TEST.MODULATE_KERNEL")):
        with pytest.raises(ValueError, match=key.replace(".", "\\.")):
            get_config(_yaml(tmp_path, f"TEST:\n  {bad}\n"))


def test_command_lines_default_to_none():
    import inference
    import validate
    for args in (validate.build_parser().parse_args(["--checkpoint", "x.pth"]), inference.build_parser().parse_args(["--input", "x.png"])):
        assert args.decode is None and args.modulate_kernel is None
    args = validate.build_parser().parse_args(["--checkpoint", "x.pth", "--decode", "unbiased", "--modulate_kernel", "17"])
    assert args.decode == "unbiased" and args.modulate_kernel == 17
    args = inference.build_parser().parse_args(["--input", "x.png", "--decode", "shift", "--sequence"])
    assert args.decode == "shift" and args.modulate_kernel is None and args.sequence
    with pytest.raises(SystemExit):
        validate.build_parser().parse_args(["--checkpoint", "x.pth", "--decode", "dark"])
    assert inference.PoseInference.decode is None and inference.PoseInference.modulate_kernel == 11


def test_decode_choice_of_the_estimator():
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    heat, fusion = types.SimpleNamespace(head_type="heatmap"), types.SimpleNamespace(head_type="fusion")
    assert PoseEstimator._decode_choice(heat, None) is False and PoseEstimator._decode_choice(heat, "shift") is False
    assert PoseEstimator._decode_choice(heat, "unbiased") is True
    assert PoseEstimator._decode_choice(fusion, None) is False and PoseEstimator._decode_choice(fusion, "shift") is False
    with pytest.raises(ValueError, match="soft-argmax"):
        PoseEstimator._decode_choice(fusion, "unbiased")
    with pytest.raises(ValueError, match="decode"):
        PoseEstimator._decode_choice(heat, "dark")


# ------------------------------------------------------------------------------------------------ the restatement on the CPU
@functools.lru_cache(maxsize=None)
def _case():
    maps, centres = unp.make_maps(200, 64, 48, seed=0)
    g = unp.taps(11)
    r64, r32 = unp.decode(maps, g, np.float64), unp.decode(maps, g, np.float32)
    maps.setflags(write=False)
    return maps, centres, r64, r32


def test_restatement_accuracy():
    maps, centres, r64, _ = _case()
    e_unb, e_shift, e_taylor = unp.mean_error(r64["coords"], centres), unp.mean_error(unp.decode_shift(maps), centres), unp.mean_error(
        unp.decode_taylor(maps), centres)
    print(f"mean error over 200 maps 64 x 48: unbiased {e_unb:.4f} px, mode 1 {e_shift:.4f} px, mode 2 {e_taylor:.4f} px")
    assert e_unb <= e_shift / 5 and e_unb <= e_taylor / 2


def test_restatement_takes_the_step_on_interior_peaks():
    _, _, r64, r32 = _case()
    inside = r64["interior"]
    share = float(r64["refined"][inside].mean())
    print(f"{int(inside.sum())} interior peaks of 200, step taken on {share:.1%}")
    assert inside.sum() >= 190 and share >= 0.95
    assert np.array_equal(r32["refined"], r64["refined"]) and np.array_equal(r32["index"], r64["index"])


def test_restatement_is_well_conditioned_in_float32():
    _, _, r64, r32 = _case()
    d = float(np.abs(r32["coords"].astype(np.float64) - r64["coords"]).max())
    print(f"float32 against float64 restatement: max difference {d:.2e} px; undecided by margin: {int((~unp.decided(r64)).sum())}")
    assert d <= 1e-5
    assert unp.decided(r64).all()


def test_restatement_leaves_degenerate_maps_at_the_integers():
    H, W = 12, 10
    maps = np.zeros((6, H, W), np.float32)
    maps[1] = 0.7
    maps[2] = -1.0 - np.random.default_rng(0).random((H, W)).astype(np.float32)
    maps[3] = unp.peak_at(H, W, 4.3, 5.2)
    maps[3, 7, 6] = np.nan
    maps[4] = unp.peak_at(H, W, 4.3, 5.2)
    maps[4, 6, 5] = np.inf
    maps[5] = unp.peak_at(H, W, 4.3, 5.2)
    for dtype in (np.float32, np.float64):
        r = unp.decode(maps, unp.taps(5), dtype)
        assert not r["refined"][:5].any() and r["refined"][5] == 1
        assert r["index"].tolist() == [0, 0, int(np.argmax(maps[2])), 7 * W + 6, 6 * W + 5, 5 * W + 4]
        assert np.array_equal(r["coords"][:5], np.stack([r["index"][:5] % W, r["index"][:5] // W], 1))
        assert np.isnan(r["maxval"][3]) and np.isinf(r["maxval"][4])
