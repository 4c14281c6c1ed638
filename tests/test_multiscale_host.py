"""Multi-scale test, host side: the numpy restatement of the merge (tests/multiscale_np.py) against identities and an affine ramp that pin
its geometry, the crop matrices (`multiscale_matrices`), the legacy-yaml mapping onto `cfg.test_scales` and the op layer's argument
errors.  Nothing here launches a kernel."""
import dataclasses

import numpy as np
import pytest
import torch

import multiscale_np as msnp

PARTNER, ramp_stack, tolerance = msnp.PARTNER, msnp.ramp_stack, msnp.tolerance


def test_single_plain_pass_is_the_identity_bitwise():
    a = np.random.default_rng(0).standard_normal((2, 3, 9, 7)).astype(np.float32)
    assert np.array_equal(msnp.merge(a, [1.0], 2).view(np.uint32), a.view(np.uint32))


def test_single_scale_flip_is_the_flip_merge_bitwise():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((2, 3, 9, 7)).astype(np.float32), rng.standard_normal((2, 3, 9, 7)).astype(np.float32)
    want = ((a + b[:, PARTNER][:, :, :, ::-1]) / np.float32(2)).astype(np.float32)
    got = msnp.merge(np.concatenate([a, b]), [1.0], 2, PARTNER, flip=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scales", [(0.75, 1.0, 1.25), (1.0, 0.5), (2.0, 1.0, 0.8)])
def test_ramp_comes_back_at_every_pixel(scales, flip):
    """Bilinear interpolation reproduces affine fields, so whichever passes see a pixel, their mean is g there: a wrong centre, a wrong
    direction of the zoom (s against 1/s), a shifted mirror or a wrong partner channel all show."""
    B, K, H, W = 2, 3, 20, 15
    stack, want = ramp_stack(scales, B, K, H, W, flip)
    got = msnp.merge(stack, scales, B, PARTNER, flip)
    err = float(np.abs(got.astype(np.float64) - want).max())
    tol = tolerance(stack, len(scales), 2 if flip else 1)
    print(f"scales {scales} flip {flip}: max error {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


def test_passes_that_cannot_see_a_pixel_do_not_dilute_it():
    """8 x 8 with (0.5, 1.0, 2.0): the inverses are exact; the scale-0.5 pass sees only the middle (u_s = 2u - 4 in [0, 7]), and u = 2 lands
    exactly on its border 0 -- inclusive."""
    H = W = 8
    stack = np.zeros((3, 1, H, W), np.float32)
    stack[0], stack[1], stack[2] = 4.0, 1.0, 2.0
    got = msnp.merge(stack, (0.5, 1.0, 2.0), 1)[0, 0]
    seen = np.array([2 <= u <= 5 for u in range(8)])                  # 2u - 4 in [0, 7]
    want = np.where(seen[:, None] & seen[None, :], np.float32(7.0) / np.float32(3.0), np.float32(1.5)).astype(np.float32)
    assert np.array_equal(got, want)
    assert float(msnp.sample_coords(8, np.float32(2.0))[2]) == 0.0


def test_multiscale_matrices_place_a_point_where_the_merge_looks_for_it():
    from infantposeestimation_gaussianbias_amd.datasets.transforms import get_affine_matrix, multiscale_matrices
    center, scale, size, hm = np.array([211.5, 140.25], np.float32), np.array([150.0, 200.0], np.float32), (96, 128), (24, 32)
    scales = (0.8, 1.0, 1.25, 2.0)
    mats = multiscale_matrices(center, scale, scales, size)
    assert len(mats) == 4 and all(m.shape == (2, 3) for m in mats)
    assert np.array_equal(mats[1], get_affine_matrix(center, scale, size, 0))
    stride = size[0] / hm[0]
    pts = np.array([[200.0, 100.0, 1.0], [260.0, 190.0, 1.0], [211.5, 140.25, 1.0]])
    base = pts @ mats[1].T / stride
    for s, m in zip(scales, mats):
        got = pts @ m.T / stride
        want = np.array([hm[0] / 2, hm[1] / 2]) + (base - np.array([hm[0] / 2, hm[1] / 2])) / s
        assert np.abs(got - want).max() < 1e-4, s                     # the matrices come from a float32 point set


def _yaml(tmp_path, text):
    p = tmp_path / "legacy.yaml"
    p.write_text("MODEL:\n  NUM_JOINTS: 13\n" + text)
    return str(p)


def test_yaml_mapping_onto_test_scales(tmp_path):
    from infantposeestimation_gaussianbias_amd.configs import Config, get_config
    assert get_config().test_scales is None and "test_scales" not in {f.name for f in dataclasses.fields(Config)}
    cfg = get_config(_yaml(tmp_path, "ADVANCED:\n  MULTI_SCALE_TEST: true\n  SCALE_LIST: [0.8, 1.0, 1.2]\n"))
    assert cfg.test_scales == (0.8, 1.0, 1.2) and cfg.data.num_keypoints == 13
    assert get_config(_yaml(tmp_path, "ADVANCED:\n  MULTI_SCALE_TEST: true\n")).test_scales == (1.0,)
    assert get_config(_yaml(tmp_path, "ADVANCED:\n  MULTI_SCALE_TEST: false\n  SCALE_LIST: [0.8, 1.0, 1.2]\n")).test_scales is None
    assert get_config(_yaml(tmp_path, "")).test_scales is None
    assert Config.test_scales is None                                  # a loaded yaml does not leak into the class
    for bad in ("[0.8, 1.2]", "[1.0, 1.0]", "[1.0, 0.0]", "[1.0, -1.5]", "[0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3]", "[]"):
        with pytest.raises(ValueError):
            get_config(_yaml(tmp_path, f"ADVANCED:\n  MULTI_SCALE_TEST: true\n  SCALE_LIST: {bad}\n"))


def test_op_layer_refuses_bad_arguments():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    st = torch.zeros(6, 3, 8, 8)
    for scales in ([0.8, 1.2], [1.0, 1.0], [1.0, float("nan")], [1.0, float("inf")], [1.0, 0.0], [1.0, -2.0], [], [1.0 + 0.1 * i for i in range(9)]):
        with pytest.raises(_lib.PoseKernelError, match="scales"):
            hipops.multiscale_merge(st, scales, 2)
    with pytest.raises(_lib.PoseKernelError, match="S\\*F\\*B"):
        hipops.multiscale_merge(st, [0.8, 1.0, 1.2], 3)                # 6 rows are not 3 * 1 * 3
    with pytest.raises(_lib.PoseKernelError, match="S\\*F\\*B"):
        hipops.multiscale_merge(st, [0.8, 1.0, 1.2], 2, torch.zeros(3, dtype=torch.int32), flip=True)      # nor 3 * 2 * 2
    with pytest.raises(_lib.PoseKernelError, match="S\\*F\\*B"):
        hipops.multiscale_merge(st[0], [1.0], 6)
    with pytest.raises(_lib.PoseKernelError, match="HIP"):
        hipops.multiscale_merge(st, [0.8, 1.0, 1.2], 2)                # a host tensor: there is no CPU implementation
    L = _lib.lib
    inv, zero = np.ones(8, np.float32), np.zeros(8, np.float32)
    one = 16                                                            # any non-null address: the checks run before anything is touched
    for args, word in (((None, None, inv.ctypes.data, one, 1, 1, 1, 1, 4, 4, None), "null"),
                       ((one, None, None, one, 1, 1, 1, 1, 4, 4, None), "null"),
                       ((one, None, inv.ctypes.data, one, 1, 2, 1, 1, 4, 4, None), "partner"),
                       ((one, None, inv.ctypes.data, one, 1, 3, 1, 1, 4, 4, None), "passes"),
                       ((one, None, inv.ctypes.data, one, 9, 1, 1, 1, 4, 4, None), "scales"),
                       ((one, None, inv.ctypes.data, one, 0, 1, 1, 1, 4, 4, None), "scales"),
                       ((one, None, inv.ctypes.data, one, 1, 1, 1, 1, 0, 4, None), "shape"),
                       ((one, None, zero.ctypes.data, one, 1, 1, 1, 1, 4, 4, None), "inverse")):
        assert L.pk_multiscale_merge(*args) == -1 and word.encode() in L.pk_last_error_string(), (args, L.pk_last_error_string())
