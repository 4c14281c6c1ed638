"""Host side of the loss-unit tests (no GPU): tests/loss_np.py against oracle/losses.py under autograd in float64 on every case of
tests/loss_cases.py, the conditions each case claims on its inputs, and a demonstration that the comparison rule and bars of
tests/test_gpu_loss_kernels.py can fail: the float32 oracle passes every case, every planted defect of loss_np.DEFECTS fails a named one.

Left out of the comparison with autograd, by rule and not by measurement:
  * pixel ties (loss_cases.tie_mask) in the heatmap gradient;
  * the coordinate gradient of a handed-in coordinate of EXACTLY 0.  torch.clamp, which the oracle's sample_border uses, passes the
    gradient when the input equals the bound (its mask is min <= x <= max), so autograd keeps the slope of the sampled offsets there;
    grid_sample(padding_mode='border') zeroes it on the bound, and that is what the kernels and loss_np state.  At those positions the
    oracle must agree with loss_np under defect='inx_always' instead, which the test asserts; at W - 1 both conventions give 0 because
    the two bilinear corners are the same pixel."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_np as ln

F64_BAR = 1e-10
RUNS = {}       # (case name, upstream name) -> (reference, oracle float64, oracle float32): computed once, never changed
INPUTS = {}


def inputs(c):
    if c.name not in INPUTS:
        INPUTS[c.name] = lc.fusion_inputs(c)
    return INPUTS[c.name]


def runs(c, up):
    key = (c.name, up[0])
    if key not in RUNS:
        x = inputs(c)
        RUNS[key] = (lc.reference(c, x, up), lc.oracle(c, x, up, torch.float64), lc.oracle(c, x, up, torch.float32))
    return RUNS[key]


def skips(c, ref, key):
    if key == "d_hm":
        return lc.tie_mask(ref["state"])
    if key == "d_coords":
        return lc.clamp_positions(inputs(c))
    return None


KEYS = ("sigma", "d_hm", "d_off", "d_var", "d_coords")


@pytest.mark.parametrize("c", lc.FUSION, ids=repr)
def test_restatement_agrees_with_autograd_in_float64(c):
    for up in lc.upstreams(c):
        ref, o64, _ = runs(c, up)
        top = max(np.abs(o64["losses"]).max(), 1e-300)
        assert np.abs(ref["losses"] - o64["losses"]).max() <= F64_BAR * top, (c, up[0], ref["losses"], o64["losses"])
        for key in KEYS:
            if ref[key] is None:
                continue
            stat = lc.map_stat(ref[key], o64[key], skips(c, ref, key))
            assert stat.max() <= F64_BAR, f"{c} / {up[0]} / {key}: {stat.max():.3g} at map {np.unravel_index(np.argmax(stat), stat.shape)}"
        on0 = lc.clamp_positions(inputs(c))
        if on0 is not None and on0.any():         # the subgradient torch takes on the bound: the slope stays (module docstring)
            other = lc.reference(c, inputs(c), up, defect="inx_always")["d_coords"]
            scale = np.abs(o64["d_coords"]).max()
            assert np.abs(other - o64["d_coords"])[on0].max() <= F64_BAR * max(scale, 1e-300)
            if up[0] == "offset":
                assert np.abs(ref["d_coords"] - o64["d_coords"])[on0].max() > 1e-3 * scale       # and the two conventions do differ there


@pytest.mark.parametrize("c", lc.FUSION, ids=repr)
def test_inputs_meet_the_conditions_their_case_claims(c):
    x = inputs(c)
    lam = np.array(lc.LAMBDAS + (lc.THRESHOLD,), np.float32)
    st = ln.fusion_forward(x["hm"], x["off"], x["var"], x["tgt"], x["w"], x["gt"], x["input_size"], lc.SIGMA_T, lam, c.utw, x["coords"])
    k = lc.conditions(c, st)
    print(f"{c}: active {k['active']:.0%}, |e| < 1 {k['small_e']:.0%}, S_k < S_o / > {k['orders']}, smallest |r - thr| {k['gap_r']:.3g}, "
          f"||e| - 1| {k['gap_e']:.3g}, |S_k - S_o| / S {k['gap_s']:.3g}, ties left out {k['tie_share']:.2%}")
    assert max(c.H, c.W) <= 64 and c.H * c.W <= 64 * 48
    assert k["gap_r"] >= 1e-3 and k["gap_e"] >= 1e-3 and k["gap_c"] >= 1e-3
    assert k["gap_s"] >= 1e-4           # float32 sums of at most 3072 sigmoids err by 1e-6 relative: the order of S_k, S_o is the same in float32
    assert k["tie_share"] <= lc.TIE_SHARE
    if "twin" in c.plants:
        assert k["tie_share"] == 0 and x["hm"][1, 0].tobytes() == x["hm"][1, 1].tobytes()
        assert st["ssum"][1, 0] == st["ssum"][1, 1] and st["ssum"][1, 1] < st["ssum"][1, 3] and (x["hm"][1, 1] == x["hm"][1, 3]).mean() > 0.9
    if "hinge" in c.claims:
        assert 0.25 <= k["active"] <= 0.75
    if "sl1" in c.claims:
        assert 0.25 <= k["small_e"] <= 0.75
    if "mixed" in c.claims:
        assert k["mixed"]
    if "orders" in c.claims:
        assert min(k["orders"]) > 0
    if "all_negative" in c.plants:
        assert st["R"][0, 0] == 0
    if "tiny_positive" in c.plants:
        assert abs(st["R"][0, 1] / (st["R"][0, 1] + 1e-8) - 2 / 3) < 1e-6 and (x["hm"][0, 1] > 0).sum() == 1
    if "w_zero_batch" in c.plants:
        assert st["S"] == 1e-8 and st["den"] == 1e-8
    if c.K == 1:
        assert st["den"] == 1e-8 and not st["pairs"]
    if c.coords:
        co, W, H = x["coords"].reshape(-1, 2), c.W, c.H
        assert (co[:, 0] == 0).any() and (co[:, 0] == W - 1).any() and (co[:, 1] == 0).any() and (co[:, 1] == H - 1).any()
        assert (co[:, 0] < 0).any() and (co[:, 0] > W - 1).any() and (co[:, 1] < 0).any() and (co[:, 1] > H - 1).any()
        assert ((co == np.round(co)).all(1) & (co > 0).all(1) & (co[:, 0] < W - 1) & (co[:, 1] < H - 1)).any()     # integer, interior


def test_case_table_covers_the_shapes():
    sizes = {(c.H, c.W) for c in lc.FUSION}
    assert sizes == {(8, 6), (16, 16), (13, 11), (16, 17), (64, 48)}
    assert {c.K for c in lc.FUSION} == {1, 2, 5, 12, 13, 17, 21}
    assert {255, 256, 257} <= {c.B * c.K for c in lc.FUSION if (c.H, c.W) == (8, 6)}
    assert any(c.B * 16 > 256 for c in lc.FUSION) and any(not c.utw for c in lc.FUSION)
    assert all(c.regime for c in lc.FUSION + lc.PIXEL + lc.STATS)
    assert max(c.B * c.K * c.H * c.W for c in lc.FUSION) == 2 * 17 * 64 * 48
    for c in lc.PIXEL:
        if c.name in lc.PIXEL_PLANS:
            total = c.B * c.K * c.HW
            assert (lc.pixel_plan(total, 1024), lc.pixel_plan(total, 2048)) == lc.PIXEL_PLANS[c.name]
    assert {c.HW for c in lc.PIXEL} >= {1, 143, 3072}


@pytest.mark.parametrize("c", lc.FUSION, ids=repr)
def test_float32_oracle_passes_the_device_bars(c):
    """the bars of the device test are M x the float32 oracle's own error, so this holds what the rule adds: exact zeros stay exact"""
    for up in lc.upstreams(c):
        ref, o64, o32 = runs(c, up)
        for key in ("losses",) + KEYS:
            if ref[key] is None:
                continue
            ratio, at, ok = lc.judge(key, o32[key], ref[key], o32[key], o64[key], skips(c, ref, key))
            assert ok, f"{c} / {up[0]} / {key}: ratio {ratio:.3g} at map {at}"
    print(f"float32 oracle passes: {c}")


FUSION_DEFECTS = [d for d in ln.DEFECTS if d not in ("pix_2w", "no_one_minus_q")]


@pytest.mark.parametrize("defect", FUSION_DEFECTS)
def test_planted_defect_fails_a_named_case(defect):
    caught = []
    for c in lc.FUSION:
        x = inputs(c)
        for up in lc.upstreams(c):
            ref, o64, o32 = runs(c, up)
            bad = lc.reference(c, x, up, defect=defect)
            for key in KEYS[1:]:
                if ref[key] is None:
                    continue
                ratio, at, ok = lc.judge(key, bad[key], ref[key], o32[key], o64[key], skips(c, ref, key) if key == "d_hm" else None)
                if not ok:
                    caught.append(f"{c} / {up[0]} / {key} map {at}: {ratio:.3g} x yardstick (bar {lc.M[key]})")
    print(f"{defect} ({ln.DEFECTS[defect]}): caught in {len(caught)} places, first: {caught[0] if caught else 'NONE'}")
    assert caught, f"no case catches '{defect}': a case is missing"


# ================================================================================================ pixel loss
@pytest.mark.parametrize("c", lc.PIXEL, ids=repr)
def test_pixel_restatement_and_bound(c):
    pred, tgt, w = c.data()
    total = pred.size
    for kind in range(4):
        terms = ln.pixel_terms(pred, tgt, w, kind)
        ref, dref = ln.pixel_loss(pred, tgt, w, kind), ln.pixel_loss_bwd(pred, tgt, w, kind)
        o_loss, o_grad = lc.pixel_oracle(pred, tgt, w, kind, torch.float64)
        assert abs(ref - o_loss) <= F64_BAR * abs(o_loss) and np.abs(dref - o_grad).max() <= F64_BAR * np.abs(o_grad).max()
        bound = lc.pixel_bound(total, terms)
        f_loss, _ = lc.pixel_oracle(pred, tgt, w, kind, torch.float32)
        assert abs(f_loss - ref) <= bound                                   # float32 on the CPU passes
        if c.name in lc.PIXEL_PLANS:                                        # the bound can fail: the last, partly empty trip lost
            last = lc.pixel_plan(total, 1024)[2]
            lost = terms.reshape(-1)[:total - last].sum() / total
            assert abs(lost - ref) > bound, f"{c} kind {kind}: losing the last trip of {last} elements stays within the bound"
    d = np.abs(pred.astype(np.float64) - tgt)
    assert (d < 1).any() and (d > 1).any() or total < 10
    if w is not None:                                                        # w w exact in float32: the 4 U of the backward counts on it
        assert (w.astype(np.float64) ** 2 == (w * w).astype(np.float64)).all()
        bad = ln.pixel_loss_bwd(pred, tgt, w, 0, defect="pix_2w")
        good = ln.pixel_loss_bwd(pred, tgt, w, 0)
        assert (np.abs(bad - good) > 4 * lc.U * np.abs(good)).any(), "pix_2w passes the 4 U bar"
        print(f"pix_2w fails: pixel / {c} / kind 0 backward")


# ================================================================================================ spatial statistics
@pytest.mark.parametrize("c", lc.STATS, ids=repr)
def test_spatial_statistics_restatement_and_defect(c):
    hm, gm, gv = c.data()
    S = hm.astype(np.float64).sum((2, 3))
    assert S[0, 0] == 0 and (hm[0, 1] > 0).sum() == 1 and abs(S[0, 2] / (S[0, 2] + 1e-8) - 0.5) < 1e-6
    mean, var = ln.spatial_stats(hm)
    d = ln.spatial_stats_bwd(hm, gm, gv)
    o64, o32 = lc.stats_oracle(hm, gm, gv, torch.float64), lc.stats_oracle(hm, gm, gv, torch.float32)
    for key, got, i in (("mean", mean, 0), ("var", var, 1), ("d_stats", d, 2)):
        assert lc.map_stat(got, o64[i]).max() <= F64_BAR, key
        assert lc.judge(key, o32[i], got, o32[i], o64[i])[2], key
    ratio, at, ok = lc.judge("d_stats", ln.spatial_stats_bwd(hm, gm, gv, defect="no_one_minus_q"), d, o32[2], o64[2])
    print(f"no_one_minus_q: spatial statistics / {c} / map {at}: {ratio:.3g} x yardstick, {'passes' if ok else 'fails'}")
    assert not ok and at[:2] == (0, 2)
