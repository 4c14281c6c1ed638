"""Feature sheets and heat-map quality on the device: pk_plane_sheet byte for byte and pk_gather_planes bit for bit against their numpy
restatement (tests/panels_np.py), pk_heatmap_quality exact in its counts, peaks and maxima and within the a-priori bound of a float64
sum in its sums, the same bits twice and on a side stream, and the public surface (feature_sheet through hrnet_w18, whose 18-channel
branches run as a 24-channel padded twin; FeatureVisualizer; HeatmapQualityAccumulator).  Small shapes only."""
import functools
import re

import numpy as np
import pytest
import torch

import panels_np as pnp
from recipe import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN, INF = np.nan, np.inf
BG = (9, 200, 31)


def G(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)           # a copy: the cached cases are read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _luts():
    return np.stack([pnp.colour_ramp(n) for n in ("sequential", "hot", "diverging")])


# ------------------------------------------------------------------------------------------------ pk_plane_sheet
@functools.lru_cache(maxsize=None)
def _planes(h, w):
    """Seven planes a and three planes b: 0 plain (negative values too), 1 constant, 2 NaN / +inf / -inf among finite values, 3 all NaN,
    4 values near 3e38 of both signs (hi - lo overflows), 5 tiny positive values, 6 one finite value among NaN."""
    g = np.random.default_rng(100 * h + w)
    a = g.standard_normal((7, h, w)).astype(np.float32)
    a[1] = -2.5
    flat = a[2].reshape(-1)
    for k, v in enumerate((NAN, INF, -INF)):
        flat[(k * 5) % flat.size] = v                            # on the 1 x 1 tile the last one stays: -inf alone
    a[3] = NAN
    a[4] = (3e38 * np.sign(a[4]) * g.uniform(0.9, 1.0, (h, w))).astype(np.float32)
    if h * w > 1:
        a[4].reshape(-1)[:2] = 3.2e38, -3.2e38
    a[5] = np.abs(a[5]) * 1e-30
    a[6] = NAN
    a[6].reshape(-1)[-1] = 7.0
    b = g.standard_normal((3, h, w)).astype(np.float32)
    b[2].reshape(-1)[0] = NAN
    a.setflags(write=False), b.setflags(write=False)
    return a, b


ALL_TILES = [(0, -1, 0), (1, -1, 0), (2, -1, 1), (3, -1, 0), (4, -1, 2), (5, -1, 1), (6, -1, 0),          # every plane, three ramps
             (0, 1, 2), (5, 0, 1), (4, 2, 0), (4, 0, 1),                                                # |a - b| with ia != ib, a NaN in b
             (7, -1, 0), (-1, -1, 0), (0, 3, 0), (0, -1, 3), (0, -1, -1), (0, -5, 1)]                   # ia, ib, ramp out of range; ib < -1 = none


def _sheet_case(h, w, tiles, cols, zoom, pad, with_b=True):
    from infantposeestimation_gaussianbias_amd import hipops
    a, b = _planes(h, w)
    if not with_b:
        b = None
    want_sheet, want_ranges = pnp.plane_sheet(a, b, tiles, _luts(), cols, zoom, pad, BG)
    SH, SW = hipops.plane_sheet_size(len(tiles), h, w, cols, zoom, pad)
    assert (SH, SW) == want_sheet.shape[:2] == pnp.sheet_size(len(tiles), h, w, cols, zoom, pad)
    sheet, ranges = hipops.plane_sheet(G(a), G(np.array(tiles, np.int32)), G(_luts()), None if b is None else G(b), cols=cols, zoom=zoom, pad=pad,
                                       background=BG)
    assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (SH, SW, 3) and ranges.dtype == torch.float32
    got_sheet, got_ranges = sheet.cpu().numpy(), ranges.cpu().numpy()
    nan_rows = np.isnan(want_ranges).all(axis=1)
    assert np.array_equal(np.isnan(got_ranges).all(axis=1), nan_rows)
    assert np.array_equal(bits(got_ranges[~nan_rows]), bits(want_ranges[~nan_rows])), (got_ranges, want_ranges)
    diff = np.argwhere((got_sheet != want_sheet).any(axis=2))
    assert diff.size == 0, f"{len(diff)} pixels differ, the first at {diff[0]}: {got_sheet[tuple(diff[0])]} != {want_sheet[tuple(diff[0])]}"
    return got_sheet, got_ranges


@pytest.mark.parametrize("h,w,cols,zoom,pad", [
    (1, 1, 4, 1, 0), (1, 1, 4, 3, 2), (1, 1, 5, 64, 2), (1, 1, 1, 64, 0),
    (3, 5, 4, 3, 2), (3, 5, 1, 1, 0), (3, 5, 17, 2, 2), (3, 5, 5, 1, 1),
    (17, 13, 4, 3, 2), (17, 13, 6, 1, 0), (17, 13, 17, 2, 1),
    (64, 48, 4, 1, 2), (64, 48, 7, 2, 0)])
def test_sheet_bytes_and_ranges_equal_the_restatement_exactly(h, w, cols, zoom, pad):
    """All seventeen tiles (T = 17 is a multiple of none of the column counts but 1 and 17: empty cells show the background)."""
    sheet, ranges = _sheet_case(h, w, ALL_TILES, cols, zoom, pad)
    if h * w > 1:
        assert float(ranges[4, 1]) - float(ranges[4, 0]) > 3.4028235e38        # the tile whose hi - lo overflows in float32 is there
    assert ranges[3, 0] == INF and ranges[3, 1] == -INF                        # all NaN: +inf, -inf
    assert np.isnan(ranges[11:16]).all() and not np.isnan(ranges[16]).any()


def test_sheet_writes_every_byte_of_a_prefilled_sheet():
    """Handed memory full of 0xAB (which no colour of this test contains), the kernel leaves none: gutters, empty cells, refused tiles."""
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    luts = _luts().copy()
    luts[luts == 0xAB] = 0xAC
    a, _ = _planes(17, 13)
    tiles = np.array([(0, -1, 0), (2, -1, 1), (9, -1, 0), (3, -1, 2), (4, -1, 0)], np.int32)
    for cols, zoom, pad in ((4, 3, 2), (5, 1, 0), (1, 2, 1), (3, 1, 1)):
        SH, SW = hipops.plane_sheet_size(5, 17, 13, cols, zoom, pad)
        guard = 64
        buf = torch.full((SH * SW * 3 + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
        sheet = buf[guard:guard + SH * SW * 3].view(SH, SW, 3)
        ranges = torch.full((5, 2), -1.0, dtype=torch.float32, device=DEV)
        _lib.call("pk_plane_sheet", G(a), 7, None, 0, G(tiles), 5, G(luts), 3, ranges, sheet, 17, 13, cols, zoom, pad, *BG, _lib.stream_ptr())
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xAB).all() and (got[-guard:] == 0xAB).all()    # nothing before or behind the sheet
        assert not (got[guard:-guard] == 0xAB).any(), (cols, zoom, pad)
        want, want_r = pnp.plane_sheet(a, None, tiles.tolist(), luts, cols, zoom, pad, BG)
        assert np.array_equal(got[guard:-guard].reshape(SH, SW, 3), want)
        assert not (ranges.cpu().numpy() == -1.0).any()


def test_sheet_without_b_and_one_ramp():
    _sheet_case(3, 5, [(0, -1, 0), (0, 0, 0), (5, -1, 0)], 2, 2, 1, with_b=False)      # ib names a plane of a b that is not there: background


def test_sheet_of_a_pixel_count_that_is_no_multiple_of_four():
    """SH SW = 3 x 3, 1 x 1, 5 x 7: the last pixels are written byte by byte."""
    for (h, w, T, cols) in ((3, 3, 1, 1), (1, 1, 1, 1), (5, 7, 1, 1), (1, 1, 3, 3)):
        from infantposeestimation_gaussianbias_amd import hipops
        a = np.arange(h * w, dtype=np.float32).reshape(1, h, w) - 2
        tiles = [(0, -1, k % 3) for k in range(T)]
        want, _ = pnp.plane_sheet(a, None, tiles, _luts(), cols, 1, 0, BG)
        sheet, _ = hipops.plane_sheet(G(a), G(np.array(tiles, np.int32)), G(_luts()), cols=cols, zoom=1, pad=0, background=BG)
        assert np.array_equal(sheet.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ pk_gather_planes
@functools.lru_cache(maxsize=None)
def _map(B, H, W, C):
    g = np.random.default_rng(B * 1000 + H * 100 + W * 10 + C)
    x = (g.standard_normal((B, H, W, C)) * np.exp2(g.integers(-8, 9, (B, H, W, C)))).astype(np.float32)
    x = G(x, torch.bfloat16)
    return x, x.float().cpu().numpy()


@pytest.mark.parametrize("B,H,W,C,c_used,b,channels", [
    (3, 5, 7, 8, 3, 0, [0, 1, 2]), (3, 5, 7, 8, 3, 2, [2, 2, 0, 3, -1, 7, 1]),
    (3, 1, 1, 8, 3, 2, [2]), (3, 1, 1, 40, 34, 0, [33, 34, 0]),
    (3, 5, 7, 40, 34, 2, list(range(34))), (3, 5, 7, 40, 34, 0, [33, 7, 8, 9, 31, 32, 33, 39, 40, -8, 0, 0, 16, 15, 24, 23, 1]),
    (1, 17, 13, 16, 16, 0, [15, 0, 8, 7])])
def test_planes_equal_the_tensor_exactly_and_guards_stay(B, H, W, C, c_used, b, channels):
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    x, x_host = _map(B, H, W, C)
    want = pnp.gather_planes(x_host, b, channels, c_used)
    n, rows = len(channels), 3
    sentinel = np.float32(-12345.5)
    buf = torch.full((rows + n * H * W + rows,), float(sentinel), dtype=torch.float32, device=DEV)
    _lib.call("pk_gather_planes", x, B, H, W, C, b, G(np.array(channels, np.int32)), n, c_used, buf[rows:], _lib.stream_ptr())
    got = buf.cpu().numpy()
    assert (got[:rows] == sentinel).all() and (got[-rows:] == sentinel).all()
    got = got[rows:-rows].reshape(n, H, W)
    for i, c in enumerate(channels):
        if 0 <= c < c_used:
            assert np.array_equal(bits(got[i]), bits(x[b, :, :, c].float().cpu().numpy())), (i, c)
        else:
            assert (bits(got[i]) == 0x7fc00000).all(), (i, c)
    assert np.array_equal(bits(got), bits(want))
    op = hipops.gather_planes(x, G(np.array(channels, np.int32)), b, c_used).cpu().numpy()
    assert np.array_equal(bits(op), bits(got))


# ------------------------------------------------------------------------------------------------ pk_heatmap_quality
def _gauss(h, w, cx, cy, sigma=1.5, amp=1.0):
    yy, xx = np.mgrid[:h, :w]
    return (amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma * sigma))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _quality_case(M, h, w):
    """Map m cycles through: 0 a Gaussian target against a shifted, scaled prediction with noise; 1 an all-zero target; 2 two equal
    maxima in both; 3 prediction == target; 4 NaN and inf in either operand; 5 a negative-only prediction; 6 two disjoint blobs."""
    g = np.random.default_rng(7 * M + h)
    P, T = np.zeros((M, h, w), np.float32), np.zeros((M, h, w), np.float32)
    for m in range(M):
        kind = m % 7
        cx, cy = g.uniform(0, w - 1), g.uniform(0, h - 1)
        T[m] = _gauss(h, w, cx, cy)
        P[m] = 0.8 * _gauss(h, w, cx + 1.3, cy - 0.7) + 0.01 * g.standard_normal((h, w)).astype(np.float32)
        if kind == 1:
            T[m] = 0
        elif kind == 2:
            T[m] = 0.25
            T[m].reshape(-1)[[h * w // 3, (2 * h * w) // 3]] = 1.0
            P[m].reshape(-1)[[h * w // 2, h * w - 1]] = 5.0
        elif kind == 3:
            P[m] = T[m]
        elif kind == 4:
            for k, v in enumerate((NAN, INF, -INF)):
                P[m].reshape(-1)[(3 * k) % (h * w)] = v
                T[m].reshape(-1)[(3 * k + 1) % (h * w)] = v
        elif kind == 5:
            P[m] = -np.abs(P[m]) - 0.5
        elif kind == 6:
            T[m], P[m] = 0, 0
            T[m, : max(1, h // 4), : max(1, w // 4)] = 1.0
            P[m, h - max(1, h // 4):, w - max(1, w // 4):] = 2.0 if h * w > 1 else 0.0
    P.setflags(write=False), T.setflags(write=False)
    rec, mag = pnp.heatmap_quality(P, T)
    return P, T, rec, mag


U = 2.0 ** -52
EXACT, SUMS = (3, 4, 5, 6, 7, 8, 9, 13, 14, 15), (0, 1, 2, 10, 11, 12)


@pytest.mark.parametrize("M,h,w", [(1, 1, 1), (2, 1, 1), (34, 1, 1), (1, 3, 5), (2, 3, 5), (34, 3, 5), (1, 64, 48), (2, 64, 48), (34, 64, 48)])
def test_quality_records_against_the_float64_restatement(M, h, w):
    from infantposeestimation_gaussianbias_amd import hipops
    P, T, want, mag = _quality_case(M, h, w)
    rec = hipops.heatmap_quality(G(P), G(T))
    assert rec.dtype == torch.float64 and tuple(rec.shape) == (M, 16)
    got = rec.cpu().numpy()
    for c in EXACT:
        assert np.array_equal(bits(got[:, c]), bits(want[:, c])), (c, got[:, c], want[:, c])
    n = h * w
    for c in SUMS:
        err, bound = np.abs(got[:, c] - want[:, c]), n * U * mag[:, c]
        print(f"column {c}: largest error {err.max():.3e}, its bound {bound[np.argmax(err)]:.3e}, bitwise equal {np.array_equal(bits(got[:, c]), bits(want[:, c]))}")
        assert np.all(err <= bound), (c, err, bound)
    for m in range(M):
        kind = m % 7
        r = got[m]
        if kind == 1:
            assert r[13] == r[14] == 0 and r[1] == 0 and r[7] == 0               # an invisible joint: no region
        if kind == 2 and n >= 3:
            assert (r[8] + w * r[9], r[5] + w * r[6]) == (n // 3, n // 2)          # the first of two equal maxima
        if kind == 3:
            assert r[2] == 0 and r[3] == 0 and r[13] == r[14] and tuple(r[4:7]) == tuple(r[7:10])
        if kind == 4:
            left_out = len({(3 * k) % n for k in range(3)} | {(3 * k + 1) % n for k in range(3)})
            assert r[15] == left_out and (left_out == n or np.isfinite(r).all())     # NaN and inf are counted and take part in nothing
        if kind == 5:
            assert r[4] < 0 and r[13] == r[14] == 0                                # a peak <= 0: no region
        if kind == 6 and n > 1:
            assert r[13] == 0 and r[14] > 0


def test_derived_quality_numbers():
    from infantposeestimation_gaussianbias_amd import utils
    P, T, want, _ = _quality_case(34, 64, 48)
    q = utils.heatmap_quality(G(P), G(T))
    same = utils.heatmap_quality(G(T), G(T))
    corr = same["correlation"].cpu().numpy()
    const = np.array([m % 7 == 1 for m in range(34)])                              # the all-zero maps: a factor is 0
    assert np.all(np.abs(corr[~const] - 1.0) <= 1e-12) and np.isnan(corr[const]).all()
    c = q["correlation"].cpu().numpy()
    assert np.isnan(c[const]).all() and np.isfinite(c[~const]).all() and np.all(np.abs(c[~const]) <= 1 + 1e-12)
    iou = q["iou_half_max"].cpu().numpy()
    kinds = np.arange(34) % 7
    assert np.all(iou[kinds == 6] == 0) and np.isnan(iou[kinds == 1]).all() and np.isnan(iou[kinds == 5]).all() and np.all(iou[kinds == 3] == 1)
    assert np.array_equal(bits(q["records"].cpu().numpy()), bits(utils.heatmap_quality(G(P), G(T))["records"].cpu().numpy()))
    r = q["records"].cpu().numpy()
    n = 64 * 48 - r[:, 15]
    assert np.allclose(q["mse"].cpu().numpy(), r[:, 2] / n, rtol=1e-15, atol=0)
    assert np.array_equal(q["peak_pred"].cpu().numpy(), r[:, [5, 6, 4]]) and np.array_equal(q["peak_gt"].cpu().numpy(), r[:, [8, 9, 7]])
    assert np.allclose(q["peak_distance"].cpu().numpy(), np.hypot(r[:, 5] - r[:, 8], r[:, 6] - r[:, 9]), rtol=1e-15)
    assert np.array_equal(q["n_nonfinite"].cpu().numpy(), r[:, 15]) and q["valid"].all()
    assert q["mse"].dtype == torch.float64 and q["mse"].is_cuda
    # (B,K,h,w) in, (B,K) out, the weight as a mask
    q4 = utils.heatmap_quality(G(P).view(2, 17, 64, 48), G(T).view(2, 17, 64, 48), weight=G(np.arange(34, dtype=np.float32).reshape(2, 17) % 3))
    assert tuple(q4["mse"].shape) == (2, 17) and tuple(q4["peak_gt"].shape) == (2, 17, 3) and tuple(q4["records"].shape) == (2, 17, 16)
    assert np.array_equal(q4["valid"].cpu().numpy().reshape(-1), np.arange(34) % 3 > 0)
    assert torch.equal(q4["records"].view(34, 16), q["records"])


# ------------------------------------------------------------------------------------------------ reproducibility
def test_same_bits_twice_and_on_a_side_stream():
    from infantposeestimation_gaussianbias_amd import hipops
    a, b = _planes(64, 48)
    P, T, _, _ = _quality_case(34, 64, 48)
    x, _ = _map(3, 5, 7, 40)
    da, db, dt, dl, dp, dg = G(a), G(b), G(np.array(ALL_TILES, np.int32)), G(_luts()), G(P), G(T)
    ch = G(np.array([33, 7, 8, 9, 40, 0], np.int32))
    torch.cuda.synchronize()

    def run():
        sheet, ranges = hipops.plane_sheet(da, dt, dl, db, cols=4, zoom=2, pad=2, background=BG)
        return sheet, ranges, hipops.gather_planes(x, ch, 1, 34), hipops.heatmap_quality(dp, dg)

    first = [t.cpu().numpy() for t in run()]
    again = [t.cpu().numpy() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run()
    torch.cuda.current_stream().wait_stream(side)
    other = [t.cpu().numpy() for t in other]
    for p, q, r in zip(first, again, other):
        assert p.tobytes() == q.tobytes() == r.tobytes()


# ------------------------------------------------------------------------------------------------ the surface
SIZE = (2, 3, 128, 96)


@functools.lru_cache(maxsize=None)
def _model():
    """hrnet_w18 with synthetic weights, as tests/test_gpu_activation.py builds it: its 18-channel branches run as a 24-channel twin."""
    import json
    import os
    from conftest import GOLDEN
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    with open(os.path.join(GOLDEN, "state_keys.json")) as f:
        keys = json.load(f)["hrnet_w18_heatmap"]
    m = PoseEstimator("hrnet_w18", 17, False, "heatmap", True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(keys, 41).items()}, strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _kept():
    """The tensors `ActivationCollector(keep_tensors=True)` keeps for one forward of the input, by layer."""
    from infantposeestimation_gaussianbias_amd import nnops, utils
    m = _model()
    x = G(synth_input("occlusion", SIZE))
    col = utils.ActivationCollector(m, keep_tensors=True)
    with torch.no_grad(), nnops.observe(col):
        m(x)
    return {name: (L.tensors[0], L.c_used) for name, L in col.layers.items()}


def _layers():
    kept = _kept()
    narrow = [n for n, (t, c) in kept.items() if t.dim() == 4 and c < t.shape[-1]]
    wide = [n for n, (t, c) in kept.items() if t.dim() == 4 and c >= 64]
    assert narrow and wide
    return narrow[-1], wide[0]


@pytest.mark.parametrize("which,channels,sample", [("narrow", 16, 0), ("narrow", 32, 1), ("narrow", [17, 0, 5, 5], 1), ("wide", 16, 1)])
def test_feature_sheet_equals_the_restatement_on_the_kept_tensor(which, channels, sample):
    """`channels=32` on the 18-channel layer is capped at 18 (no tapped layer of this model has fewer than 16 real channels, so the cap is
    shown one step up); the twin's six padding channels are never shown."""
    from infantposeestimation_gaussianbias_amd import utils
    m = _model()
    layer = _layers()[0 if which == "narrow" else 1]
    t, c_used = _kept()[layer]
    x = G(synth_input("occlusion", SIZE))
    before = x.clone()
    sheet, ranges, shown = utils.feature_sheet(m, x, layer, channels=channels, sample=sample, cols=4, zoom=2, pad=2)
    want_list = list(range(min(channels, c_used))) if isinstance(channels, int) else channels
    assert shown == want_list and (which != "narrow" or c_used == 18 and t.shape[-1] == 24)
    planes = pnp.gather_planes(t.float().cpu().numpy(), sample, shown, c_used)
    want, want_r = pnp.plane_sheet(planes, None, [(i, -1, 0) for i in range(len(shown))], pnp.colour_ramp("sequential"), 4, 2, 2, (255, 255, 255))
    assert np.array_equal(sheet.cpu().numpy(), want) and np.array_equal(bits(ranges.cpu().numpy()), bits(want_r))
    assert torch.equal(x, before) and not x.requires_grad and not m.training


def test_feature_sheet_zoom_mode_and_refusals():
    from infantposeestimation_gaussianbias_amd import utils
    m = _model()
    narrow, wide = _layers()
    x = G(synth_input("occlusion", SIZE))[:1]
    sheet, ranges, shown = utils.feature_sheet(m, x, narrow)                      # zoom None: as large as fits into 2048 per side
    t, _ = _kept()[narrow]
    H, W = int(t.shape[1]), int(t.shape[2])
    zoom = int(sheet.shape[0] - 2 - 4 * 2) // (4 * H)
    assert len(shown) == 16 and tuple(sheet.shape) == (2 + 4 * (H * zoom + 2), 2 + 4 * (W * zoom + 2), 3) and tuple(ranges.shape) == (16, 2)
    assert max(sheet.shape[:2]) <= 2048 and (max(2 + 4 * (H * (zoom + 1) + 2), 2 + 4 * (W * (zoom + 1) + 2)) > 2048 or zoom == 64)
    m.train()
    try:
        utils.feature_sheet(m, x, narrow, channels=2, zoom=1)
        assert m.training                                                         # the caller's mode comes back
        with pytest.raises(ValueError, match="the tapped layers are: .*" + re.escape(narrow)):
            utils.feature_sheet(m, x, "backbone.no_such_layer")
        assert m.training
    finally:
        m.eval()
    with pytest.raises(ValueError, match="outside 0 .. 17"):
        utils.feature_sheet(m, x, narrow, channels=[0, 18])
    with pytest.raises(ValueError, match="sample 1 of a batch of 1"):
        utils.feature_sheet(m, x, narrow, sample=1)
    with pytest.raises(TypeError):
        utils.feature_sheet(m, x.cpu(), narrow)
    col = utils.FeatureCollector(m, [narrow])
    from infantposeestimation_gaussianbias_amd import nnops
    with torch.no_grad(), nnops.observe(col):
        m(G(synth_input("occlusion", SIZE)))
    assert list(col.features) == [narrow] and narrow in col.seen and wide in col.seen and not col.layers      # nothing reduced
    feat, c_used = col.feature(narrow)
    assert c_used == 18 and torch.equal(feat, _kept()[narrow][0])


def test_feature_visualizer_returns_the_kind_that_came_in():
    from infantposeestimation_gaussianbias_amd import utils
    g = np.random.default_rng(5)
    f = g.standard_normal((2, 6, 9, 7)).astype(np.float32)
    want, _ = pnp.plane_sheet(f[0], None, [(i, -1, 0) for i in range(6)], pnp.colour_ramp("sequential"), 4, 64, 2, (255, 255, 255))
    out_np = utils.FeatureVisualizer.visualize_feature_maps(f, "layer", num_samples=16)
    assert isinstance(out_np, np.ndarray) and out_np.dtype == np.uint8 and np.array_equal(out_np, want)
    out_dev = utils.FeatureVisualizer.visualize_feature_maps(G(f), "layer")
    assert isinstance(out_dev, torch.Tensor) and out_dev.is_cuda and np.array_equal(out_dev.cpu().numpy(), want)
    assert utils.FeatureVisualizer.visualize_feature_maps(f[0], "layer") is None        # the reference's answer to a shape that is not 4-D
    t, c_used = _kept()[_layers()[0]]                                                    # a tapped (B,H,W,C) bf16 map
    tapped = utils.FeatureVisualizer.visualize_feature_maps(t, "tapped", num_samples=3)
    H, W = int(t.shape[1]), int(t.shape[2])
    zoom = (int(tapped.shape[0]) - 4) // H
    planes = pnp.gather_planes(t.float().cpu().numpy(), 0, [0, 1, 2], int(t.shape[-1]))
    want_t, _ = pnp.plane_sheet(planes, None, [(i, -1, 0) for i in range(3)], pnp.colour_ramp("sequential"), 4, zoom, 2, (255, 255, 255))
    assert tapped.is_cuda and np.array_equal(tapped.cpu().numpy(), want_t)
    # the three-column heat-map figure
    P, T, _, _ = _quality_case(2, 3, 5)
    luts = np.stack([pnp.colour_ramp("hot"), pnp.colour_ramp("diverging")])
    tiles = [t3 for j in range(2) for t3 in ((j, -1, 0), (2 + j, -1, 0), (2 + j, j, 1))]
    sheet, ranges = utils.heatmap_quality_sheet(G(P), G(T), zoom=3, pad=1)
    want_q, want_r = pnp.plane_sheet(np.concatenate([T, P]), T, tiles, luts, 3, 3, 1, (255, 255, 255))
    assert np.array_equal(sheet.cpu().numpy(), want_q) and tuple(ranges.shape) == (2, 3, 2)
    assert np.array_equal(bits(ranges.cpu().numpy().reshape(6, 2)), bits(want_r))
    fig_np = utils.FeatureVisualizer.visualize_heatmap_quality(P, T, ["a", "b"])
    fig_dev = utils.FeatureVisualizer.visualize_heatmap_quality(G(P), G(T), ["a", "b"])
    assert isinstance(fig_np, np.ndarray) and fig_dev.is_cuda and np.array_equal(fig_np, fig_dev.cpu().numpy())
    assert fig_np.shape[1] == 2 + 3 * (5 * (fig_np.shape[0] - 2 - 2 * 2) // (2 * 3) + 2)
    with pytest.raises(ValueError, match="1 joint names for 2 maps"):
        utils.FeatureVisualizer.visualize_heatmap_quality(P, T, ["a"])


def test_accumulator_over_two_batches_equals_the_concatenation():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd.utils.feature_maps import quality_report_json
    P, T, want, _ = _quality_case(34, 3, 5)
    K = 2
    P4, T4 = P.reshape(17, K, 3, 5), T.reshape(17, K, 3, 5)
    weight = (np.arange(34).reshape(17, K) % 5 > 0).astype(np.float32)              # every fifth map is an invisible joint
    acc = utils.HeatmapQualityAccumulator(K)
    acc.update(G(P4[:6]), G(T4[:6]), G(weight[:6]))
    acc.update(G(P4[6:]), G(T4[6:]), G(weight[6:])[:, :, None])                    # the loader's (B,K,1) weight
    rep = acc.compute()
    whole = utils.heatmap_quality(G(P4), G(T4), G(weight))
    assert np.array_equal(bits(rep["records"]), bits(whole["records"].cpu().numpy())) and rep["n_samples"] == 17 and rep["map_size"] == [3, 5]
    valid = weight > 0
    for name in ("mse", "peak_distance", "correlation", "iou_half_max", "mass_ratio", "max_abs_diff"):
        v = whole[name].cpu().numpy()
        for k in range(K):
            col = v[valid[:, k], k]
            col = col[~np.isnan(col)]
            got = rep["joints"][k][name]
            assert (np.isnan(got) and col.size == 0) or abs(got - col.mean()) <= 1e-12 * max(1.0, abs(col.mean())), (name, k)
        pooled = v[valid]
        pooled = pooled[~np.isnan(pooled)]
        assert abs(rep["pooled"][name] - pooled.mean()) <= 1e-12 * max(1.0, abs(pooled.mean())), name
    assert [j["n"] for j in rep["joints"]] == valid.sum(axis=0).tolist() and rep["pooled"]["n"] == int(valid.sum())
    # a weight-0 map changes nothing, whatever it holds
    P2 = P4.copy()
    P2[~valid] = 1e30
    acc2 = utils.HeatmapQualityAccumulator(K)
    acc2.update(G(P2), G(T4), G(weight))
    rep2 = acc2.compute()
    assert quality_report_json(rep2) == quality_report_json(rep)
    import json
    text = json.dumps(quality_report_json(rep))
    assert "NaN" not in text and "records" not in json.loads(text)
    with pytest.raises(ValueError, match="after maps of"):
        acc.update(G(P4[:1, :, :2]), G(T4[:1, :, :2]))


# ------------------------------------------------------------------------------------------------ front ends
def test_validate_accumulates_the_quality_of_the_loss_forward(tmp_path):
    """`validate(heatmap_quality=...)`: the metrics are unchanged, the accumulator gets the loss forward's heat maps against the loader's
    target and weight, the JSON and the sheet of the first sample are written."""
    import json
    import logging
    import validate as V
    from PIL import Image
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import SyntheticLoader
    cfg = get_config("hrnet_w18")
    cfg.train.batch_size = 2
    log, dev = logging.getLogger("test"), torch.device(DEV)
    seen = []

    class Recording(utils.HeatmapQualityAccumulator):
        def update(self, pred, gt, weight=None):
            assert all(torch.is_tensor(t) and t.is_cuda for t in (pred, gt, weight)) and pred.shape == gt.shape
            seen.append(tuple(t.detach().float().clone() for t in (pred, gt, weight)))
            return super().update(pred, gt, weight)

    m = _model()
    plain, _ = V.validate(m, SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False)
    acc, path, png = Recording(17), tmp_path / "q.json", tmp_path / "sheet.png"
    with_q, _ = V.validate(m, SyntheticLoader(cfg, n_batches=2), dev, cfg, log, flip_test=False, heatmap_quality=acc,
                           heatmap_quality_report=str(path), heatmap_quality_sheet=str(png))
    assert set(with_q) == set(plain)
    for k in plain:
        assert with_q[k] == plain[k] or (np.isnan(with_q[k]) and np.isnan(plain[k])), k
    assert len(seen) == 2 and all(tuple(s[0].shape[:2]) == (2, 17) and s[2].numel() == 34 for s in seen)
    pred, gt, weight = (torch.cat([s[i] for s in seen]) for i in range(3))
    whole = utils.heatmap_quality(pred, gt, weight.reshape(4, 17))
    rep = acc.compute()
    assert np.array_equal(bits(rep["records"]), bits(whole["records"].cpu().numpy())) and rep["n_samples"] == 4
    with open(path) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(utils.feature_maps.quality_report_json(rep))) and len(back["joints"]) == 17 and "records" not in back
    valid = (weight.reshape(4, 17) > 0).cpu().numpy()
    assert [j["n"] for j in back["joints"]] == valid.sum(axis=0).tolist() and back["pooled"]["n"] == int(valid.sum()) > 0
    h, w = int(pred.shape[2]), int(pred.shape[3])
    want, _ = utils.heatmap_quality_sheet(pred[0], gt[0])
    drawn = np.asarray(Image.open(png).convert("RGB"))[:, :, ::-1]
    assert drawn.shape[0] >= 17 * h and drawn.shape[1] >= 3 * w and np.array_equal(drawn, want.cpu().numpy())
    # maps of another shape than the target's are refused with both shapes named; so is a loader of detector boxes
    with pytest.raises(RuntimeError, match=r"\(2, 17, 8, 6\).*\(2, 17, 4, 6\)"):
        V._update_heatmap_quality(utils.HeatmapQualityAccumulator(17), {"heatmaps": torch.zeros(2, 17, 8, 6, device=DEV)},
                                  {"target": torch.zeros(2, 17, 4, 6), "target_weight": torch.ones(2, 17, 1)}, dev, None)

    class Boxes:
        dataset = None

        def __iter__(self):
            z = torch.zeros
            yield {"img": z(1, 3, cfg.data.input_size[1], cfg.data.input_size[0]),
                   "meta": {"box_score": torch.ones(1), "center": z(1, 2), "scale": torch.ones(1, 2), "image_id": [1], "ann_id": [1],
                            "area": [1.0], "bbox": z(1, 4)}}

        def __len__(self):
            return 1

    with pytest.raises(RuntimeError, match="heat-map quality needs ground-truth targets"):
        V.validate(m, Boxes(), dev, cfg, log, flip_test=False, heatmap_quality=utils.HeatmapQualityAccumulator(17))


def test_feature_map_switch_writes_the_sheet_and_prints_the_ranges(tmp_path, capsys):
    import argparse
    import inference
    from PIL import Image
    from infantposeestimation_gaussianbias_amd import utils
    torch.manual_seed(11)
    pose = inference.PoseInference(config="hrnet_w18", flip_test=False)
    img = np.random.default_rng(12).integers(0, 256, (120, 160, 3)).astype(np.uint8)
    bbox = np.array([20.0, 10.0, 140.0, 110.0])
    out = tmp_path / "features.png"
    args = argparse.Namespace(feature_maps="backbone.bn2", feature_channels=[5, 0, 63], feature_zoom=2, output=str(out))
    sheet, ranges, shown = inference.main_feature_maps(args, pose, img, bbox)
    text = capsys.readouterr().out
    x, _, _ = pose.preprocess(img, bbox)
    want, want_r, _ = utils.feature_sheet(pose.model, x, "backbone.bn2", channels=[5, 0, 63], zoom=2)
    assert shown == [5, 0, 63] and torch.equal(sheet, want) and torch.equal(ranges, want_r)
    assert "Feature maps of backbone.bn2: 3 channels" in text and all(f"channel {c:4d}:" in text for c in shown)
    assert np.array_equal(np.asarray(Image.open(out).convert("RGB"))[:, :, ::-1], sheet.cpu().numpy())
    first = inference.main_feature_maps(argparse.Namespace(**{**vars(args), "feature_channels": [4], "feature_zoom": None}), pose, img, bbox)
    assert first[2] == [0, 1, 2, 3] and max(first[0].shape[:2]) <= 2048
    with pytest.raises(ValueError, match="the tapped layers are"):
        inference.main_feature_maps(argparse.Namespace(**{**vars(args), "feature_maps": "nowhere"}), pose, img, bbox)
