"""Feature sheets and heat-map quality, host side (no GPU): the declarations of the new entries, their refusals in the documented order
through ctypes, the colour ramps, the numpy restatement (tests/panels_np.py) on hand-computed cases, and the new flags of inference.py and
validate.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import panels_np as pnp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _lib():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ declarations
def test_the_header_declares_the_entries_with_their_argument_types():
    decl = _lib().declared_symbols()
    assert decl["pk_gather_planes"] == ("int", [P, I, I, I, I, I, P, I, I, P, P])
    assert decl["pk_plane_sheet_size"] == ("int", [I, I, I, I, I, I, P, P])
    assert decl["pk_plane_sheet"] == ("int", [P, I, P, I, P, I, P, I, P, P, I, I, I, I, I, I, I, I, P])
    assert decl["pk_heatmap_quality"] == ("int", [P, P, P, I64, I, I, P])
    const = _lib().CONSTANTS
    assert (const["PK_PANEL_MAX_TILES"], const["PK_PANEL_MAX_SIDE"], const["PK_PANEL_MAX_PLANE"]) == (4096, 8192, 1 << 24)
    assert (const["PK_PANEL_MAX_ZOOM"], const["PK_PANEL_MAX_PAD"], const["PK_QUALITY_COLS"]) == (64, 64, 16)
    for name in decl:
        assert "tsne" not in name


# ------------------------------------------------------------------------------------------------ refusals
# Argument checks run before anything touches the device, so a made-up non-null address is never read.
X = 0x1000


def refused(name, *args):
    L = _lib().lib
    rc = getattr(L, name)(*args)
    assert rc == -1, (name, args, rc)
    return L.pk_last_error_string().decode()


def size(T, h, w, cols, zoom, pad):
    SH, SW = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = _lib().lib.pk_plane_sheet_size(T, h, w, cols, zoom, pad, ctypes.addressof(SH), ctypes.addressof(SW))
    return rc, SH.value, SW.value


def test_gather_planes_refuses_in_the_documented_order():
    ok = dict(x=X, B=2, H=5, W=7, C=8, b=0, ch=X, n=3, c_used=3, out=X)

    def go(**kw):
        a = {**ok, **kw}
        return refused("pk_gather_planes", a["x"], a["B"], a["H"], a["W"], a["C"], a["b"], a["ch"], a["n"], a["c_used"], a["out"], None)

    for k in ("x", "ch", "out"):
        assert "null pointer" in go(**{k: None, "C": 12, "H": 0})           # null first, whatever else is wrong
    assert "bad shape" in go(H=0, C=12)                                       # the shape before C % 8
    assert "bad shape" in go(H=4097, W=4096)                                  # H W beyond 2^24
    assert "not a multiple of 8" in go(C=12, b=5)                             # C % 8 before the sample
    assert "sample 2 of 2" in go(b=2, n=0) and "sample -1" in go(b=-1)
    assert "0 planes" in go(n=0, c_used=0) and "4097 planes" in go(n=4097)
    assert "c_used=9" in go(c_used=9, x=X + 2) and "c_used=0" in go(c_used=0)
    assert "aligned" in go(x=X + 8) and "aligned" in go(out=X + 2) and "aligned" in go(ch=X + 1)


def test_plane_sheet_size_limits_and_their_order():
    L = _lib().lib
    assert L.pk_plane_sheet_size(5, 3, 5, 4, 3, 2, None, None) == -1 and b"null pointer" in L.pk_last_error_string()
    assert size(5, 3, 5, 4, 3, 2) == (0, 24, 70)                              # rows = 2: 2 + 2 (9 + 2), 2 + 4 (15 + 2)
    assert size(1, 1, 1, 1, 1, 0) == (0, 1, 1) and size(1, 1, 1, 1, 64, 64) == (0, 192, 192)
    assert size(4096, 1, 1, 64, 1, 0) == (0, 64, 64) and size(3, 2, 2, 3, 1, 0) == (0, 2, 6) and size(3, 2, 2, 1, 1, 0) == (0, 6, 2)
    assert size(1, 128, 1, 1, 64, 0) == (0, 8192, 64) and size(1, 1, 8192, 1, 1, 0) == (0, 1, 8192)      # 8192 accepted
    for args, text in (((0, 3, 5, 4, 3, 2), "0 tiles"), ((4097, 3, 5, 4, 3, 2), "4097 tiles"), ((5, 0, 5, 4, 3, 2), "bad tile"),
                       ((5, 4097, 4096, 4, 3, 2), "bad tile"), ((5, 3, 5, 0, 3, 2), "cols=0"), ((5, 3, 5, 4, 0, 2), "zoom=0"),
                       ((5, 3, 5, 4, 65, 2), "zoom=65"), ((5, 3, 5, 4, 3, 65), "pad=65"), ((5, 3, 5, 4, 3, -1), "pad=-1"),
                       ((1, 1, 8193, 1, 1, 0), "1 x 8193"), ((1, 8193, 1, 1, 1, 0), "8193 x 1"), ((1, 128, 1, 1, 64, 1), "8194 x 66"),
                       ((0, 0, 0, 0, 0, 65), "0 tiles"), ((5, 3, 5, 0, 0, 65), "cols=0"), ((5, 3, 5, 4, 0, 65), "zoom=0")):
        rc, SH, SW = size(*args)
        assert rc == -1 and (SH, SW) == (-7, -7), args                        # a refusal writes nothing
        assert text in L.pk_last_error_string().decode(), (args, L.pk_last_error_string())


def test_plane_sheet_refuses_in_the_documented_order():
    ok = dict(a=X, Na=2, b=None, Nb=0, tiles=X, T=5, luts=X, L=1, ranges=X, sheet=X, h=3, w=5, cols=4, zoom=3, pad=2, bg=(255, 255, 255))

    def go(**kw):
        a = {**ok, **kw}
        return refused("pk_plane_sheet", a["a"], a["Na"], a["b"], a["Nb"], a["tiles"], a["T"], a["luts"], a["L"], a["ranges"], a["sheet"],
                       a["h"], a["w"], a["cols"], a["zoom"], a["pad"], *a["bg"], None)

    for k in ("a", "tiles", "luts", "ranges", "sheet"):
        assert "null pointer" in go(**{k: None, "T": 0})                      # null first
    assert "0 tiles" in go(T=0, Na=0) and "4097 tiles" in go(T=4097)          # then what the size query refuses, under this entry's name
    assert go(T=0).startswith("pk_plane_sheet:")
    assert "zoom=0" in go(zoom=0, Na=0) and "zoom=65" in go(zoom=65) and "pad=65" in go(pad=65)
    assert "bad tile" in go(h=4097, w=4096, T=1, cols=1, zoom=1, pad=0)       # h w beyond 2^24
    assert "1 x 8193" in go(T=1, cols=1, h=1, w=8193, zoom=1, pad=0, Na=0)
    assert "bad counts" in go(Na=0, bg=(256, 0, 0)) and "bad counts" in go(L=0) and "bad counts" in go(Nb=-1)
    assert "b is NULL" in go(Nb=2)                                            # planes announced, none given
    assert "background" in go(bg=(256, 0, 0), a=X + 1) and "background" in go(bg=(0, -1, 0))
    assert "aligned" in go(a=X + 2) and "aligned" in go(sheet=X + 1) and "aligned" in go(b=X + 2, Nb=1)


def test_heatmap_quality_refuses_in_the_documented_order():
    def go(pred=X, gt=X, rec=X, M=2, h=3, w=5):
        return refused("pk_heatmap_quality", pred, gt, rec, M, h, w, None)

    for k in ("pred", "gt", "rec"):
        assert "null pointer" in go(**{k: None, "M": 0})
    assert "bad shape" in go(M=0, pred=X + 1) and "bad shape" in go(h=0) and "bad shape" in go(w=-1)
    assert "bad shape" in go(h=4097, w=4096)
    assert "aligned" in go(pred=X + 2) and "aligned" in go(gt=X + 1) and "aligned" in go(rec=X + 4)


def test_ops_refuse_cpu_tensors():
    import torch
    from infantposeestimation_gaussianbias_amd import hipops, utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    z = torch.zeros(2, 3, 5)
    with pytest.raises(PoseKernelError):
        hipops.heatmap_quality(z, z)
    with pytest.raises(PoseKernelError):
        hipops.plane_sheet(z, torch.zeros(1, 3, dtype=torch.int32), torch.zeros(256, 3, dtype=torch.uint8))
    with pytest.raises(PoseKernelError):
        hipops.gather_planes(torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(PoseKernelError):
        utils.heatmap_quality(z, z)
    with pytest.raises(PoseKernelError):
        utils.HeatmapQualityAccumulator(2).update(z[None], z[None])
    assert not hasattr(utils.FeatureVisualizer, "visualize_feature_tsne")


# ------------------------------------------------------------------------------------------------ ramps
ANCHORS = {"hot": {0: (0, 0, 0), 255: (255, 255, 255)},
           "sequential": {0: (68, 1, 84), 255: (253, 231, 37)},
           "diverging": {0: (59, 76, 192), 255: (180, 4, 38)}}


@pytest.mark.parametrize("name", ["hot", "sequential", "diverging", "jet"])
def test_ramps_have_their_shape_and_anchor_colours(name):
    from infantposeestimation_gaussianbias_amd.utils.visualization import colour_ramp, heatmap_lut
    lut = colour_ramp(name)
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and lut.flags["C_CONTIGUOUS"]
    assert np.array_equal(lut, pnp.colour_ramp(name))
    rgb = lut[:, ::-1].astype(np.int64)                                       # the tables are BGR
    for i, colour in ANCHORS.get(name, {}).items():
        assert tuple(rgb[i]) == colour, (name, i, rgb[i])
    if name == "jet":
        assert np.array_equal(lut, heatmap_lut())
    if name in ("hot", "sequential"):
        luma = 0.299 * rgb[:, 0] + 0.587 * rgb[:, 1] + 0.114 * rgb[:, 2]
        assert np.all(np.diff(luma) >= 0), name


def test_inner_anchors_fall_between_the_table_entries_that_bracket_them():
    """t = 1/4, 1/2, 3/4 are no table entries (255 t is no integer there): the entries on either side bracket the anchor colour."""
    from infantposeestimation_gaussianbias_amd.utils.visualization import colour_ramp
    for name, inner in (("sequential", {0.25: (59, 82, 139), 0.5: (33, 145, 140), 0.75: (94, 201, 98)}), ("diverging", {0.5: (221, 221, 221)})):
        rgb = colour_ramp(name)[:, ::-1].astype(np.int64)
        for t, colour in inner.items():
            lo, hi = int(np.floor(255 * t)), int(np.ceil(255 * t))
            for c in range(3):
                assert min(rgb[lo, c], rgb[hi, c]) - 1 <= colour[c] <= max(rgb[lo, c], rgb[hi, c]) + 1, (name, t, c)
    # 'hot' at the ends of its three segments: red full at t = 0.365079, green at 0.746032
    hot = colour_ramp("hot")[:, ::-1]
    assert hot[94, 0] == 255 and hot[92, 0] < 255 and hot[93, 1] == 0 and hot[191, 1] == 255 and hot[190, 2] == 0 and hot[191, 2] > 0
    with pytest.raises(ValueError, match="viridis"):
        colour_ramp("viridis")


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_sheet_geometry_by_hand():
    assert pnp.sheet_size(5, 3, 5, 4, 3, 2) == (24, 70)
    a = np.zeros((5, 3, 5), np.float32)
    for t in range(5):
        a[t] = np.arange(15, dtype=np.float32).reshape(3, 5) * (t + 1)
    lut = np.stack([np.arange(256)] * 3, axis=1).astype(np.uint8)              # grey: the byte is the index
    tiles = [(t, -1, 0) for t in range(5)]
    sheet, ranges = pnp.plane_sheet(a, None, tiles, lut, 4, 3, 2, (9, 8, 7))
    assert sheet.shape == (24, 70, 3) and np.array_equal(ranges, np.array([[0, 14 * (t + 1)] for t in range(5)], np.float32))
    assert np.all(sheet[:2] == (9, 8, 7)) and np.all(sheet[:, :2] == (9, 8, 7)) and np.all(sheet[11:13] == (9, 8, 7))
    assert np.all(sheet[13:, 19:] == (9, 8, 7))                               # three empty cells of the last row and its gutters
    # tile 0: origin (2, 2); element (i, j) covers a 3 x 3 block; index floor(255 v / (14 + 1e-8)) in float32
    for (i, j) in ((0, 0), (0, 1), (1, 2), (2, 4)):
        v = np.float32(5 * i + j)
        want = int(np.floor(np.float32(255) * (v / (np.float32(14) + np.float32(1e-8)))))
        assert np.all(sheet[2 + 3 * i:5 + 3 * i, 2 + 3 * j:5 + 3 * j] == min(want, 255)), (i, j)
    assert sheet[10, 16, 0] == 255 and sheet[2, 2, 0] == 0
    # tile 4: row 1, column 0 -> origin (13, 2); tile 3: row 0, column 3 -> origin (2, 53)
    assert sheet[13 + 8, 2 + 14, 0] == 255 and sheet[12, 2, 0] == 9 and sheet[2 + 8, 53 + 14, 0] == 255 and sheet[2, 52, 0] == 9


def test_index_rule_on_constant_nonfinite_and_overflowing_tiles():
    idx, lo, hi = pnp.tile_index(np.full((3, 5), 2.5, np.float32))
    assert not idx.any() and lo == hi == np.float32(2.5)                      # a constant tile: 0 / 1e-8 everywhere
    nan, inf = np.nan, np.inf
    idx, lo, hi = pnp.tile_index(np.array([[nan, -1.0, inf], [3.0, -inf, 1.0]], np.float32))
    assert (lo, hi) == (-1.0, 3.0) and idx.tolist() == [[0, 0, 0], [255, 0, 127]]
    idx, lo, hi = pnp.tile_index(np.full((2, 2), nan, np.float32))
    assert lo == np.inf and hi == -np.inf and not idx.any()
    idx, lo, hi = pnp.tile_index(np.array([[-3e38, 3e38, 0.0, 1e38]], np.float32))
    assert not idx.any()                                                      # hi - lo overflows: finite / inf = 0, inf / inf = NaN -> 0
    idx, _, _ = pnp.tile_index(np.array([[0.0, 1.0, 0.5, 1e-9]], np.float32))
    assert idx.tolist() == [[0, 255, 127, 0]]                                 # 1 + 1e-8 rounds to 1 in float32: the maximum reaches 255
    sheet, ranges = pnp.plane_sheet(np.zeros((1, 1, 1), np.float32), None, [(0, -1, 0), (1, -1, 0), (0, 0, 0), (0, -1, 1)],
                                    np.zeros((256, 3), np.uint8), 4, 1, 0, (5, 5, 5))
    assert np.isnan(ranges[1:]).all() and np.all(sheet[0, 1:] == 5) and np.all(sheet[0, 0] == 0)


def test_quality_records_by_hand():
    g = np.zeros((1, 3, 5), np.float32)
    g[0, 1, 2], g[0, 1, 3] = 1.0, 0.5
    p = np.zeros((1, 3, 5), np.float32)
    p[0, 1, 3], p[0, 2, 3], p[0, 0, 0] = 2.0, 2.0, np.nan
    rec, mag = pnp.heatmap_quality(p, g)
    r = rec[0]
    assert (r[0], r[1], r[2], r[3]) == (4.0, 1.5, 1.0 + 2.25 + 4.0, 2.0)
    assert tuple(r[4:7]) == (2.0, 3.0, 1.0) and tuple(r[7:10]) == (1.0, 2.0, 1.0)      # the first of the two equal maxima
    assert (r[13], r[14], r[15]) == (1.0, 3.0, 1.0)                           # p >= 1: two cells; g >= 0.5: two cells; one shared
    mp, mg = 4.0 / 14, 1.5 / 14
    assert abs(r[11] - (2 * (2 - mp) ** 2 + 12 * mp ** 2)) < 1e-12 and abs(r[12] - ((1 - mg) ** 2 + (0.5 - mg) ** 2 + 12 * mg ** 2)) < 1e-12
    assert mag[0, 0] == 4.0 and mag[0, 2] == 7.25
    # the ordered sum is a sum: exact on integers, whatever the order
    v = np.arange(1000, dtype=np.float64)
    assert pnp.ordered_sum((v, np.ones(1000, bool))) == 499500.0 and pnp.ordered_sum((v, v % 2 == 0)) == 249500.0


# ------------------------------------------------------------------------------------------------ scripts
def _script(name):
    import importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(name)


def test_inference_parses_the_feature_map_flags():
    p = _script("inference").build_parser()
    ns = p.parse_args(["--input", "a.png", "--output", "s.png", "--feature_maps", "backbone.bn2", "--feature_channels", "3", "5", "8",
                       "--feature_zoom", "4"])
    assert (ns.feature_maps, ns.feature_channels, ns.feature_zoom) == ("backbone.bn2", [3, 5, 8], 4)
    ns = p.parse_args(["--input", "a.png", "--output", "s.png", "--feature_maps", "backbone.bn2"])
    assert ns.feature_channels is None and ns.feature_zoom is None
    ns = p.parse_args(["--input", "a.png"])
    assert ns.feature_maps is None
    for bad in (["--feature_maps", "x"],                                       # no --output
                ["--output", "s.png", "--feature_channels", "4"], ["--output", "s.png", "--feature_zoom", "2"],
                ["--output", "s.png", "--feature_maps", "x", "--feature_zoom", "65"],
                ["--output", "s.png", "--feature_maps", "x", "--grad_cam", "0"],
                ["--output", "s.png", "--feature_maps", "x", "--sequence"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--input", "a.png"] + bad)


def test_validate_parses_the_heatmap_quality_flags():
    p = _script("validate").build_parser()
    ns = p.parse_args(["--checkpoint", "c.pth", "--heatmap_quality", "q.json", "--heatmap_quality_sheet", "s.png"])
    assert (ns.heatmap_quality, ns.heatmap_quality_sheet) == ("q.json", "s.png")
    ns = p.parse_args(["--checkpoint", "c.pth"])
    assert ns.heatmap_quality is None and ns.heatmap_quality_sheet is None
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint", "c.pth", "--heatmap_quality_sheet", "s.png"])
