"""Unbiased (DARK) decode on the device: pk_unbiased_decode against the float64 restatement of its specification (tests/unbiased_np.py,
which blurs the whole map where the kernel blurs a patch) at the shapes where the kernel can go wrong, degenerate maps, the accuracy
against modes 1 and 2, reproducibility (two launches, hipGraph replay) and the layers above: PoseEstimator.inference /
inference_multiscale(decode=), get_max_preds_unbiased, the fusion head's refusal and validate(decode=)."""
import functools

import numpy as np
import pytest
import torch

import unbiased_np as unp
from recipe import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(i, i + 1) for i in range(1, 17, 2)]
TOL = 1e-4          # px: the project's fixture tolerance; the float32-to-float64 spread of the restatement is 4e-6 px at 11 taps, 7e-6 at 31

# (H, W), ksize, border of the generator (0: centres anywhere on the map, the border included).  BK = 34 each.
#   9 x 7, k 11: the map is smaller than the kernel in both axes and has fewer pixels (63) than the workgroup has threads
#   20 x 15: 300 pixels, the strided argmax loop wraps with a ragged tail
#   5 x 5, k 3: exactly one interior position;  4 x 4: none, the step is never taken
#   64 x 48 and 128 x 128 (k 11 and 17; 31 is the largest patch): the real map sizes
CASES = [((9, 7), 11, 0.0), ((20, 15), 11, 0.0), ((20, 15), 5, 0.0), ((5, 5), 3, 0.0), ((4, 4), 3, 0.0), ((64, 48), 11, 4.0), ((128, 128), 11, 4.0),
         ((128, 128), 17, 4.0), ((64, 48), 31, 4.0)]


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached inputs are read-only


def C(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _restated(hw, k, border, n=34, seed=7):
    maps, centres = unp.make_maps(n, hw[0], hw[1], seed, border=border)
    maps.setflags(write=False)
    g = unp.taps(k)
    return maps, centres, unp.decode(maps, g, np.float64), unp.decode(maps, g, np.float32)


def _device(maps, k, shape=None):
    from infantposeestimation_gaussianbias_amd import hipops
    n, H, W = maps.shape
    idx, mv, co, ref = hipops.unbiased_decode(G(maps).view(*(shape or (2, n // 2)), H, W), k)
    return C(idx).reshape(n), C(mv).reshape(n), C(co).reshape(n, 2), C(ref).reshape(n)


def _compare(maps, r64, r32, got, what):
    """index and maxval exact; the restatement well conditioned (asserted first, so a bad input fails as a bad input); refined exact and
    coords within TOL of float64 wherever no decision hangs on the last bits; at most 10 % of the maps excluded."""
    idx, mv, co, ref = got
    spread = float(np.abs(r32["coords"].astype(np.float64) - r64["coords"]).max())
    ok = unp.decided(r64)
    assert spread <= 1e-5 and np.array_equal(r32["refined"][ok], r64["refined"][ok]), (what, spread)
    assert (~ok).sum() <= 0.1 * len(ok), (what, int((~ok).sum()))
    assert np.array_equal(idx, r64["index"]) and idx.dtype == np.int32
    assert np.array_equal(mv.view(np.uint32), r64["maxval"].view(np.uint32))
    assert ref.dtype == np.uint8 and np.array_equal(ref[ok], r64["refined"][ok])
    err = float(np.abs(co[ok].astype(np.float64) - r64["coords"][ok]).max())
    print(f"{what}: {len(ok)} maps, {int((~ok).sum())} excluded for margin, {int(r64['refined'].sum())} steps taken, float32 restatement spread "
          f"{spread:.2e} px, max |kernel - float64 restatement| {err:.2e} px")
    assert err <= TOL
    still = ok & (r64["refined"] == 0)
    assert np.array_equal(co[still], r64["coords"][still].astype(np.float32))          # exactly the integers where no step is taken


@pytest.mark.parametrize("hw,k,border", CASES)
def test_kernel_equals_the_float64_restatement(hw, k, border):
    maps, _, r64, r32 = _restated(hw, k, border)
    _compare(maps, r64, r32, _device(maps, k), f"{hw} k={k}")
    n_in = int(r64["interior"].sum())
    if hw == (4, 4):
        assert n_in == 0 and not r64["refined"].any()
    elif hw == (5, 5):
        assert 0 < n_in < 34 and all(i == 2 * 5 + 2 for i in r64["index"][r64["interior"]])
    elif border == 0.0:
        assert 0 < n_in < 34                   # both sides of the interior rule are exercised
    else:
        assert r64["refined"].mean() >= 0.95


@pytest.mark.parametrize("k", [5, 11])
def test_step_is_taken_at_2_and_size_minus_3_only(k):
    """Noise-free peaks placed by hand at px in {0, 1, 2, W-3, W-2, W-1} and likewise in y, sigma 1.5 and 2.0: the step is taken only at 2
    and size - 3, where the zero padding is inside the stencil's blur."""
    H, W = 20, 15
    maps, want = [], []
    for sigma in (1.5, 2.0):
        for axis, n in (("x", W), ("y", H)):
            for p in (0, 1, 2, n - 3, n - 2, n - 1):
                maps.append(unp.peak_at(H, W, p + 0.2, 9.3, sigma) if axis == "x" else unp.peak_at(H, W, 7.3, p - 0.2, sigma))
                want.append(int(p in (2, n - 3)))
    maps = np.stack(maps)
    g = unp.taps(k)
    r64, r32 = unp.decode(maps, g, np.float64), unp.decode(maps, g, np.float32)
    assert r64["refined"].tolist() == want and unp.decided(r64).all()
    placed = [(p, 9) for p in (0, 1, 2, W - 3, W - 2, W - 1)] + [(7, p) for p in (0, 1, 2, H - 3, H - 2, H - 1)]
    assert [(int(i % W), int(i // W)) for i in r64["index"]] == placed * 2
    got = _device(maps, k)
    _compare(maps, r64, r32, got, f"border peaks k={k}")
    assert got[3].tolist() == want


def _degenerate(H, W):
    rng = np.random.default_rng(3)
    maps = np.zeros((6, H, W), np.float32)
    maps[1] = 0.7                                                      # constant
    maps[2] = -1.0 - rng.random((H, W)).astype(np.float32)             # all negative
    maps[3] = unp.peak_at(H, W, 4.3, 5.2)
    maps[3, 7, 6] = np.nan                                             # one NaN, away from the peak: it is the maximum
    maps[4] = unp.peak_at(H, W, 4.3, 5.2)
    maps[4, 6, 5] = np.inf                                             # one +inf
    # two-way tie: 1.0 at (x 4, y 1), where no step may be taken, and 1.0 at the top of a peak centred on (5, 6), where one would be
    maps[5] = unp.peak_at(H, W, 5.0, 6.0)
    maps[5, 1, 4] = 1.0
    assert maps[5, 6, 5] == 1.0 and (maps[5] == 1.0).sum() == 2
    want_idx = [0, 0, int(np.argmax(maps[2])), 7 * W + 6, 6 * W + 5, 1 * W + 4]
    return maps, want_idx


@pytest.mark.parametrize("k", [3, 11])
def test_degenerate_maps_stay_at_the_integer_argmax(k):
    H, W = 12, 10
    maps, want_idx = _degenerate(H, W)
    r64 = unp.decode(maps, unp.taps(k), np.float64)
    assert not r64["refined"].any() and r64["index"].tolist() == want_idx          # the specification itself says so
    idx, mv, co, ref = _device(maps, k)
    assert idx.tolist() == want_idx and not ref.any()
    assert np.array_equal(co, np.stack([idx % W, idx // W], 1).astype(np.float32))
    assert np.isnan(mv[3]) and mv[4] == np.inf and mv[5] == 1.0
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(mv[keep].view(np.uint32), maps.reshape(6, -1)[keep, idx[keep]].view(np.uint32))
    # the tie the other way round: the interior maximum first, the step is taken there
    flipped = np.ascontiguousarray(maps[5:6, ::-1, ::-1])
    r = unp.decode(flipped, unp.taps(k), np.float64)
    idx2, _, co2, ref2 = _device(np.concatenate([flipped, flipped]), k)
    assert r["refined"][0] == 1 and ref2.tolist() == [1, 1] and idx2[0] == r["index"][0] == (H - 1 - 6) * W + (W - 1 - 5)
    assert np.abs(co2[0] - r["coords"][0]).max() <= TOL


def test_accuracy_on_the_device():
    """The 200 maps of the host test (64 x 48, peaks of sigma 1.5 / 2.0, noise 0.02): the unbiased decode's mean error is at most a fifth
    of mode 1's and at most half of mode 2's, all three decoded on the device."""
    from infantposeestimation_gaussianbias_amd import hipops
    maps, centres = unp.make_maps(200, 64, 48, seed=0)
    hm = G(maps).view(8, 25, 64, 48)
    unb = C(hipops.unbiased_decode(hm, 11)[2]).reshape(200, 2)
    m1, m2 = (C(hipops.argmax_decode(hm, mode)[2]).reshape(200, 2) for mode in (1, 2))
    e_unb, e1, e2 = unp.mean_error(unb, centres), unp.mean_error(m1, centres), unp.mean_error(m2, centres)
    print(f"mean error on the device over 200 maps 64 x 48: unbiased {e_unb:.4f} px, mode 1 {e1:.4f} px, mode 2 {e2:.4f} px")
    assert e_unb <= e1 / 5 and e_unb <= e2 / 2


def test_two_launches_and_graph_replay_give_identical_bytes():
    """Eager twice, then flip merge + decode captured into a hipGraph (the tail of served inference: the capture refuses a host
    synchronisation or a host-to-device copy) and replayed on two inputs."""
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    maps = [G(unp.make_maps(34, 64, 48, seed=s)[0]).view(2, 17, 64, 48) for s in (11, 12, 13)]
    a, b = hipops.unbiased_decode(maps[0], 11), hipops.unbiased_decode(maps[0], 11)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    partner = torch.arange(17, dtype=torch.int32)
    for i, j in PAIRS:
        partner[i], partner[j] = j, i
    partner = partner.to(DEV)
    tail = lambda h, hf: PoseEstimator.decode_heatmaps(hipops.flip_merge(h, hf, partner), unbiased=True, kernel=11)
    want = [tail(maps[i], maps[2]) for i in (0, 1)]
    static = maps[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        tail(static, maps[2])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = tail(static, maps[2])
    torch.cuda.current_stream().wait_stream(s)
    for i in (0, 1, 0):
        static.copy_(maps[i])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[i][0]) and torch.equal(out[1], want[i][1])
    assert not torch.equal(want[0][0], want[1][0])


def test_optional_outputs_and_empty_batches():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    maps = G(unp.make_maps(34, 20, 15, seed=5)[0])
    idx, mv, co, ref = hipops.unbiased_decode(maps.view(2, 17, 20, 15), 5)
    only = torch.empty(34, 2, device=DEV)
    _lib.call("pk_unbiased_decode", maps, unp.taps(5).ctypes.data, 5, None, None, only, None, 34, 20, 15, _lib.stream_ptr())
    assert torch.equal(only, co.view(34, 2))
    out = hipops.unbiased_decode(torch.empty(0, 17, 20, 15, device=DEV), 5)
    assert [tuple(t.shape) for t in out] == [(0, 17), (0, 17), (0, 17, 2), (0, 17)]
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.float32, torch.uint8]


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


def test_inference_decodes_the_merged_heatmaps():
    from infantposeestimation_gaussianbias_amd import hipops
    m = _model("hrnet_w18")
    x = G(synth_input("ms_one", (2, 3, 128, 96)))
    with torch.no_grad():
        both = m(torch.cat([x, torch.flip(x, dims=[-1])], 0))["heatmaps"].float()
    merged = hipops.flip_merge(both[:2], both[2:], m._flip_partner(PAIRS, x.device))
    _, mv, co, ref = hipops.unbiased_decode(merged, 11)
    kp, sc = m.inference(x, True, PAIRS, decode="unbiased")
    assert kp.shape == (2, 17, 2) and torch.equal(kp, co) and torch.equal(sc, mv)
    kp0, sc0 = m.inference(x, True, PAIRS)
    assert torch.equal(sc, sc0) and not torch.equal(kp, kp0)                      # same maxima, other coordinates at some joint
    assert bool(ref.any()) and bool(((kp - kp0).abs().amax(-1) > 0)[ref.bool()].any())
    kp5, _ = m.inference(x, True, PAIRS, decode="unbiased", modulate_kernel=5)
    assert torch.equal(kp5, hipops.unbiased_decode(merged, 5)[2]) and not torch.equal(kp5, kp)
    # None and 'shift' are today's decode, bit for bit
    for flip, pairs in ((True, PAIRS), (False, None)):
        today = m.decode_heatmaps(merged if flip else both[:2])
        for decode in (None, "shift"):
            got = m.inference(x, flip, pairs, decode=decode)
            assert torch.equal(got[0], today[0]) and torch.equal(got[1], today[1])
    assert torch.equal(today[0], hipops.argmax_decode(both[:2], 1)[2])
    with pytest.raises(ValueError, match="decode"):
        m.inference(x, True, PAIRS, decode="dark")


def test_inference_multiscale_decodes_the_merged_heatmaps():
    from infantposeestimation_gaussianbias_amd import hipops
    m, scales, B = _model("hrnet_w18"), (0.8, 1.25, 1.0), 2
    xs = [G(synth_input(f"ms_{i}", (B, 3, 128, 96))) for i in range(3)]
    with torch.no_grad():
        hms = m(torch.cat([t for x in xs for t in (x, torch.flip(x, dims=[-1]))], 0))["heatmaps"].float()
    merged = hipops.multiscale_merge(hms, scales, B, m._flip_partner(PAIRS, xs[0].device), True)
    _, mv, co, _ = hipops.unbiased_decode(merged, 11)
    kp, sc = m.inference_multiscale(xs, scales, True, PAIRS, decode="unbiased")
    assert torch.equal(kp, co) and torch.equal(sc, mv)
    today = m.decode_heatmaps(merged)
    assert not torch.equal(kp, today[0])
    for decode in (None, "shift"):
        got = m.inference_multiscale(xs, scales, True, PAIRS, decode=decode)
        assert torch.equal(got[0], today[0]) and torch.equal(got[1], today[1])
    kp17, _ = m.inference_multiscale(xs, scales, True, PAIRS, decode="unbiased", modulate_kernel=17)
    assert torch.equal(kp17, hipops.unbiased_decode(merged, 17)[2])


def test_get_max_preds_unbiased_has_the_shapes_of_its_siblings():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd.utils import postprocess as pp
    hm = G(unp.make_maps(34, 64, 48, seed=2)[0]).view(2, 17, 64, 48)
    preds, mv = pp.get_max_preds_unbiased(hm)
    p0, mv0 = pp.get_max_preds(hm)
    p2, mv2 = pp.get_max_preds_with_subpixel(hm)
    assert preds.shape == p0.shape == p2.shape == (2, 17, 2) and mv.shape == mv0.shape == mv2.shape == (2, 17, 1)
    assert preds.dtype == p0.dtype and torch.equal(mv, mv0)
    assert torch.equal(preds, hipops.unbiased_decode(hm, 11)[2]) and torch.equal(pp.get_max_preds_unbiased(hm, kernel=5)[0], hipops.unbiased_decode(hm, 5)[2])
    assert float((preds - p0).abs().max()) <= 2.0 and not torch.equal(preds, p0)
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    decoded, m_dec = PoseEstimator.decode_heatmaps(hm, unbiased=True)
    assert torch.equal(decoded, preds) and torch.equal(m_dec, mv.squeeze(-1))


def test_fusion_head_refuses_the_unbiased_decode():
    m = _model("hrformer_small")
    x = G(synth_input("ms_one", (2, 3, 128, 96)))
    with pytest.raises(ValueError, match="soft-argmax"):
        m.inference(x, True, PAIRS, decode="unbiased")
    with pytest.raises(ValueError, match="soft-argmax"):
        m.inference_multiscale([x], [1.0], True, PAIRS, decode="unbiased")
    kp, sc = m.inference(x, True, PAIRS, decode="shift")                           # today's behaviour: the head's own decode
    kp0, sc0 = m.inference(x, True, PAIRS)
    assert torch.equal(kp, kp0) and torch.equal(sc, sc0)


def test_validate_runs_with_the_unbiased_decode(tmp_path):
    """Three small images with two persons each behind the COCO loader (the set-up of test_gpu_multiscale.py): validate(decode='unbiased')
    reports the ten COCO numbers, from the predictions of inference(decode='unbiased'); the argument wins over the config, the config is
    used when no argument is given, and nothing set is today's run."""
    import json
    import logging
    import os

    from PIL import Image

    import coco_cases as cc
    import validate as V
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import build_dataloader
    from infantposeestimation_gaussianbias_amd.utils.coco_eval import STAT_KEYS
    from infantposeestimation_gaussianbias_amd.utils.postprocess import heatmap_to_image_coords
    rng = np.random.default_rng(0)
    os.makedirs(tmp_path / "val")
    images, anns = [], []
    for i in range(3):
        H, W = 160 + 20 * i, 140 + 10 * i
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp_path / "val" / f"{i}.png")
        images.append({"id": 100 + i, "file_name": f"{i}.png", "width": W, "height": H})
        for j in range(2):
            anns.append(cc.gt_ann(1 + 2 * i + j, 100 + i, cc.pose(17, 20 + 50 * j, 30, 60, rng), 60 * 60 * 0.8 + 3000 * j, bbox=[15 + 50 * j, 25, 70, 70]))
    (tmp_path / "ann.json").write_text(json.dumps({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}))
    cfg = get_config("hrnet_w18")
    cfg.data.data_root, cfg.data.val_ann, cfg.data.val_img_prefix = str(tmp_path), "ann.json", "val/"
    cfg.data.train_ann, cfg.data.train_img_prefix = "ann.json", "val/"
    cfg.train.batch_size, cfg.train.num_workers = 2, 0
    model, log, dev = _model("hrnet_w18"), logging.getLogger("test"), torch.device(DEV)
    loader = build_dataloader(cfg, is_train=False)
    plain, preds0 = V.validate(model, loader, dev, cfg, log, flip_test=True)
    metrics, preds = V.validate(model, loader, dev, cfg, log, flip_test=True, decode="unbiased")
    assert set(STAT_KEYS) <= set(metrics) and len(STAT_KEYS) == 10 and set(metrics) == set(plain)
    assert all(np.isfinite(metrics[k]) for k in STAT_KEYS) and metrics["loss"] == plain["loss"] and len(preds) == len(preds0) == 6
    assert any(p["keypoints"] != q["keypoints"] for p, q in zip(preds, preds0))
    want = []
    for batch in loader:
        kp, sc = model.inference(batch["img"].to(dev), True, cfg.data.flip_pairs, decode="unbiased")
        xy = heatmap_to_image_coords(kp, batch["meta"]["center"].to(dev), batch["meta"]["scale"].to(dev), cfg.data.input_size, cfg.data.heatmap_size)
        want += [np.concatenate([xy[b].cpu().numpy(), sc[b].cpu().numpy()[:, None]], 1).reshape(-1).tolist() for b in range(kp.shape[0])]
    assert [p["keypoints"] for p in preds] == want
    cfg.decode, cfg.modulate_kernel = "unbiased", 11
    _, preds_c = V.validate(model, loader, dev, cfg, log, flip_test=True)                         # from the config
    assert [p["keypoints"] for p in preds_c] == want
    _, preds_a = V.validate(model, loader, dev, cfg, log, flip_test=True, decode="shift")         # the argument wins
    assert [p["keypoints"] for p in preds_a] == [p["keypoints"] for p in preds0]
    cfg.modulate_kernel = 10
    with pytest.raises(ValueError, match="modulate_kernel"):
        V.validate(model, loader, dev, cfg, log, flip_test=True)
