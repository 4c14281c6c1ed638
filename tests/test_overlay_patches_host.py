"""Host-side checks of the per-person heatmap overlay (no GPU): the entry points are declared and exported and refuse bad arguments
before anything touches a device, the heat-map matrix is the crop matrix it is documented to be, and the inputs of the GPU comparison
(tests/test_gpu_overlay_patches.py) meet that test's conditions when evaluated on the float64 restatement alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_patches_np as opn  # noqa: E402


def test_patch_overlay_entry_points_are_declared_exported_and_check_their_arguments():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    for name in ("pk_heatmap_overlay_patches", "pk_heatmap_overlay_patches_ws_floats"):
        assert name in decl and hasattr(_lib.lib, name), name
    L = _lib.lib
    # the workspace: one max plane per patch plus its min and max
    assert L.pk_heatmap_overlay_patches_ws_floats(256, 17, 64, 48) == 256 * 64 * 48 + 2 * 256
    assert L.pk_heatmap_overlay_patches_ws_floats(1, 13, 8, 6) == 48 + 2
    assert L.pk_heatmap_overlay_patches_ws_floats(0, 17, 64, 48) == 0
    assert L.pk_heatmap_overlay_patches_ws_floats(65535, 1, 8192, 8192) == 0            # does not fit an int
    q = 1 << 20                                           # never dereferenced: every call below fails its checks

    def call(images=q, hm=q, idx=q, mat=q, alpha=0.5, lut=q, ws=q, N=1, P=1, K=17, h=8, w=8, H=16, W=16):
        return L.pk_heatmap_overlay_patches(images, hm, idx, mat, alpha, lut, None, None, ws, N, P, K, h, w, H, W, None)
    for missing in ("images", "hm", "idx", "mat", "lut", "ws"):
        assert call(**{missing: None}) == -1 and b"null pointer" in L.pk_last_error_string(), missing
    for bad in (dict(N=0), dict(N=65536), dict(P=0), dict(K=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0)):
        assert call(**bad) == -1 and b"bad shape" in L.pk_last_error_string(), bad
    assert call(P=65536) == -1 and b"65535" in L.pk_last_error_string()
    for bad in (dict(H=8193), dict(W=8193), dict(h=8193), dict(w=8193)):
        assert call(**bad) == -1 and b"8192" in L.pk_last_error_string(), bad
    assert call(P=65535, h=8192, w=8192) == -1 and b"workspace" in L.pk_last_error_string()
    assert call(alpha=float("nan")) == -1 and b"NaN" in L.pk_last_error_string()


@pytest.mark.parametrize("rot", [0.0, 30.0])
def test_heat_map_matrix_is_the_crop_matrix_scaled_to_the_heat_map(rot):
    """Heat pixel x is input pixel x w_in / w (the decode's convention), so the map from image to heat pixels is the crop matrix with the
    heat-map size as its output size, and equally diag(w / w_in, h / h_in) times the crop matrix of the network's input.  Both sides come
    out of a float64 solve of the same well-conditioned 6 x 6 system (entries of a few hundred) with right-hand sides that differ by the
    exact factor 1/4: they agree to a few ulps of the entries, far inside 1e-9."""
    from infantposeestimation_gaussianbias_amd.datasets.transforms import get_affine_matrix
    from infantposeestimation_gaussianbias_amd.utils.visualization import crop_heatmap_matrices
    (w_in, h_in), (w, h) = (192, 256), (48, 64)
    center, scale = np.array([163.25, 201.5]), np.array([150.0, 200.0])
    heat = get_affine_matrix(center, scale, (w, h), rot)
    crop = get_affine_matrix(center, scale, (w_in, h_in), rot)
    assert np.allclose(heat, np.diag([w / w_in, h / h_in]) @ crop, rtol=0, atol=1e-9)
    assert np.array_equal(crop_heatmap_matrices([center], [scale], (w, h), [rot])[0], heat)
    # the centre of the crop is the centre of the heat map, and one crop width spans w heat pixels along the rotated axis
    assert np.allclose(heat @ np.array([center[0], center[1], 1.0]), [w / 2, h / 2], atol=1e-9)
    assert np.isclose(np.hypot(heat[0, 0], heat[1, 0]), w / scale[0], atol=1e-9)


def test_inputs_of_the_gpu_comparison_meet_its_conditions():
    """No mapped pixel centre within 1e-6 heat pixels of a patch edge (so float64 on the device and here decide `covered` alike), and
    under 0.5 % of the covered pixels within 1e-3 of an integer 255 v (the band in which a float32 index may differ by one).  Also that
    the inputs are the situations the comparison is meant to hold: overlap, an empty frame, a rotated patch, one cut by the frame, one
    inside a single tile."""
    N, H, W = opn.FRAMES
    big, tiny = opn.comparison_cases()
    for case in (big, tiny):
        mats = opn.case_matrices(case)
        covered = banded = 0
        covers = []
        for n in range(N):
            v, cover, edge = opn.overlay_patches_f64(H, W, case["heatmaps"], case["image_index"], mats, n)
            assert edge.min() > 1e-6, f"frame {n}: a pixel centre maps within {edge.min():.3g} heat pixels of a patch edge"
            on = cover > 0
            assert not np.isnan(v[on]).any() and np.isnan(v[~on]).all()
            covered += int(on.sum())
            banded += int((np.abs(v[on] - np.rint(v[on])) <= 1e-3).sum())
            covers.append(cover)
        share = banded / covered
        print(f"P = {len(mats)}: {covered} covered pixels, share within 1e-3 of an integer 255 v: {share:.5f}")
        assert share < 0.005
        if case is big:
            assert covers[0].max() == 2 and (covers[0] == 1).any() and covers[1].max() == 0 and covers[2].max() >= 1
            ys, xs = np.nonzero(opn.overlay_patches_f64(H, W, case["heatmaps"][4:], [2], mats[4:], 2)[1])
            assert len(ys) > 0 and xs.min() // 32 == xs.max() // 32 and ys.min() // 8 == ys.max() // 8, "the small patch spans tiles"
            cut = opn.overlay_patches_f64(H, W, case["heatmaps"][3:4], [2], mats[3:4], 2)[1]
            assert cut[:, W - 1].any() and cut[0].any() and 0 < cut.sum() < 0.9 * 66 * 88, "the fourth patch is not cut by the frame"
            rot = opn.overlay_patches_f64(H, W, case["heatmaps"][2:3], [2], mats[2:3], 2)[1]
            ys, xs = np.nonzero(rot)
            assert rot.sum() < 0.8 * (np.ptp(xs) + 1) * (np.ptp(ys) + 1), "the rotated patch fills its bounding box"
        else:
            assert covers[1].max() == 1 and covers[0].max() == 0 and covers[2].max() == 0


def test_restatement_of_the_rule_on_a_case_done_by_hand():
    """A 2 x 2 plane shifted by half a pixel: the covered pixel carries the mean of its four taps, normalised to the plane's own range."""
    hm = np.array([[[[0.0, 1.0], [2.0, 4.0]]]], np.float32)
    mat = np.array([[1.0, 0.0, -1.5, 0.0, 1.0, -2.5]])               # frame (2, 3) -> heat (0.5, 0.5)
    v, cover, edge = opn.overlay_patches_f64(6, 5, hm, [0], mat, 0)
    assert cover.sum() == 1 and cover[3, 2] == 1 and np.isclose(v[3, 2], 255.0 * 1.75 / (4.0 + 1e-8)) and np.isclose(edge[3, 2], 0.5)
    assert opn.index_of(v, cover)[3, 2] == 111 and opn.index_of(v, cover).sum() == 111
    assert opn.overlay_patches_f64(6, 5, hm, [0], mat, 1)[1].sum() == 0
