"""The loss unit (csrc/pk_loss.hip: k_floss_map, k_floss_pair, k_floss_final, k_floss_sigma, k_floss_bwd, the pixel losses and the
spatial statistics with their backward) per term and per map against float64, on the cases of tests/loss_cases.py: every case is the
smallest shape that reaches its regime and says which (hinge on and off around one joint, |e| on both sides of 1, maps of 48 / 143 /
256 / 272 / 3072 pixels, B K = 255 / 256 / 257, B 16 > 256 pairs, K = 1 / 2 / 12 / 21, an all-negative map, a 2e-8 map, bit-identical
partner maps, zero and half weights, use_target_weight off, coordinates handed in on, at and beyond the border, pixel-loss grids that wrap).

Reference: tests/loss_np.py (float64, closed-form backward written from the header), which tests/test_loss_host.py holds against
oracle/losses.py under autograd to 1e-10 per map.  The surface is hipops.fusion_terms / fusion_loss / pixel_loss / spatial_stats; the
guard tests call the C entries so that outputs and workspace can lie inside larger allocations.

Rule (loss_cases.judge): every map is judged alone, max |got - ref| over the map / the map's largest |ref|; a map whose reference is
identically zero must be identically zero; d_offsets is zero wherever the reference is (all but the bilinear corners).  A map passes at
M x the same statistic of the float32 CPU evaluation of oracle/losses.py (floored at 2^-20).  M per tensor is loss_cases.M: the smallest
power of two at least twice the largest ratio of one run on an MI355X.  Largest ratios of that run, per tensor (upstream, case):

    the seven values   0.61  (peak, 64x48 K17)                     M = 2
    sigma              2.39  (64x48 K17, map (0, 15))              M = 8
    d_heatmaps         13    (variance one-hot, 8x6 K1 B257, map (47, 0)); 12 (peak one-hot, 13x11 K5 unweighted, (1, 4));
                             10.6 (offset one-hot, 8x6 K17 B17, (16, 11)); 9.3 (random 7-vector); 5.1 (3 x total); 1.04 (overlap one-hot);
                             0.54 (shape one-hot); 0.17 (heatmap one-hot)                                              M = 32
    d_offsets          6.06  (offset one-hot, 8x6 K1 B257, map (153, 0))  M = 16
    d_variances        1.61  (variance one-hot, 8x6 K17 B17, map (4, 7))  M = 4
    d_coords           0.97  (random 7-vector with grad_sigma, 13x11 K17 coords, map (0, 12))  M = 2
    spatial statistics mean 0.16, var 1.0, gradient 0.26                  M = 1, 2, 1

The ratios above 8 are all in d_heatmaps and have one cause, read off the workspace of those maps (DESIGN.md "Loss kernels: test bars"):
the soft-argmax coordinate c = sx / z is 2 to 3 ulp off (the CPU's within one), and the backward uses c in differences that cancel --
pixel - c next to the peak (peak term), qx - c QSUM, two centroids 0.019 px apart (variance term), e = o(c) - (g - c) at |e| = 0.1
(offset term).  The pixel loss reached 0.083 of its bound for the value and 0.78 of 4 U for the gradient.

The pixel loss has a derived bound instead (loss_cases docstring): (k + 2) 2^-24 sum|term| / count for the value, 4 x 2^-24 relative
per element for the gradient.  The module prints the largest ratio per tensor and upstream at its end."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_np as ln

gpu = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024
GUARD_BITS = 0x5A5AA5A5        # as a float 1.5e16: no kernel here produces it
KEYS = ("losses", "sigma", "d_hm", "d_off", "d_var", "d_coords")
WORST = {}          # (tensor, upstream) -> (largest ratio to the yardstick, case, map)
RUNS = {}           # (case, upstream) -> (reference, oracle float64, oracle float32): computed once, never changed
INPUTS = {}


@pytest.fixture(scope="module")
def ops():
    from infantposeestimation_gaussianbias_amd import _lib, hipops
    yield hipops, _lib
    print()
    for (key, up), (ratio, case, at) in sorted(WORST.items()):
        print(f"{key:9s} {up:14s} largest ratio to the float32 yardstick {ratio:8.3g}  ({case}, map {at})  bar {lc.M.get(key, '-')}")


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


def dev(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def host(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def record(key, up, ratio, case, at):
    if ratio > WORST.get((key, up), (-1.0,))[0]:
        WORST[(key, up)] = (ratio, str(case), at)


def device_run(hipops, c, x, up):
    _, lam, g, gs, via = up
    hm, off, var, co = dev(x["hm"], True), dev(x["off"], True), dev(x["var"], True), dev(x["coords"], True)
    tgt, w, gt = dev(x["tgt"]), dev(x["w"]), dev(x["gt"])
    if via == "loss":
        losses = hipops.fusion_loss(hm, off, var, tgt, w, gt, x["input_size"], lc.SIGMA_T, dev(lam), c.utw)
        sigma = None
        (3.0 * losses[6]).backward()
    else:
        losses, sigma = hipops.fusion_terms(dev(lam), hm=hm, off=off, var=var, coords=co, target=tgt, weight=w, gt=gt,
                                            input_size=x["input_size"], sigma_t=lc.SIGMA_T, use_target_weight=c.utw)
        obj = (losses * dev(g)).sum()
        if gs is not None:
            obj = obj + (sigma * dev(gs)).sum()
        obj.backward()
    torch.cuda.synchronize()
    return dict(losses=host(losses), sigma=host(sigma), d_hm=host(hm.grad), d_off=host(off.grad), d_var=host(var.grad),
                d_coords=None if co is None else host(co.grad))


def hold(c, upname, got, ref, o64, o32, failures):
    for key in KEYS:
        if ref[key] is None or got[key] is None:
            continue
        assert not np.isnan(got[key]).any(), f"{c} / {upname} / {key}: NaN"
        skip = lc.tie_mask(ref["state"]) if key == "d_hm" else None
        ratio, at, ok = lc.judge(key, got[key], ref[key], o32[key], o64[key], skip)
        record(key, upname, ratio, c, at)
        print(f"{c} / {upname} / {key}: {ratio:.3g} x yardstick at map {at}")
        if not ok:
            failures.append(f"{c} / {upname} / {key}: {ratio:.3g} x the float32 yardstick at map {at}, bar {lc.M[key]}")
    stray = (ref["d_off"] == 0) & (got["d_off"] != 0)
    if stray.any():
        failures.append(f"{c} / {upname}: d_offsets non-zero off the bilinear corners at {np.argwhere(stray)[0]}")


@gpu
@pytest.mark.parametrize("c", lc.FUSION, ids=repr)
def test_fusion_terms_per_term_and_map(ops, c):
    hipops, _ = ops
    x = inputs(c)
    failures = []
    for up in lc.upstreams(c):
        ref, o64, o32 = runs(c, up)
        hold(c, up[0], device_run(hipops, c, x, up), ref, o64, o32, failures)
    assert not failures, "\n".join(failures)


# ================================================================================================ guards
def guarded(n, dtype=torch.float32):
    """-> (buffer, view of n elements holding NaN between two guards of GUARD elements holding GUARD_BITS)"""
    buf = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + n].view(dtype)
    view.fill_(float("nan"))
    return buf, view


def guards_hold(buf, n):
    return bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[GUARD + n:] == GUARD_BITS).all())


def fusion_c_entries(L, c, x, up, plain):
    """one forward and backward through the C entries into guarded outputs -> {name: (buffer, view)}; grad_total = 3 on the device"""
    B, K, H, W = c.B, c.K, c.H, c.W
    _, lam, g, gs, _ = up
    n = B * K * H * W
    hm, off, var, tgt, w, gt, co = (dev(x[k]) for k in ("hm", "off", "var", "tgt", "w", "gt", "coords"))
    sizes = dict(ws=B * K * 24 + B * 16 * 4 + 16, losses=7, sigma=B * K, d_hm=n, d_off=2 * n, d_var=n, d_coords=2 * B * K)
    out = {k: guarded(v) for k, v in sizes.items()}
    v = {k: b[1] for k, b in out.items()}
    st = L.stream_ptr()
    g3 = dev(np.array([3.0], np.float32))
    if plain:
        L.call("pk_fusion_loss_fwd", hm, off, var, tgt, w, gt, v["ws"], v["losses"], B, K, H, W, x["input_size"][0], x["input_size"][1],
               lc.SIGMA_T, dev(lam), int(c.utw), st)
        L.call("pk_fusion_loss_bwd", hm, off, var, tgt, w, v["ws"], g3, v["d_hm"], v["d_off"], v["d_var"], B, K, H, W, lc.SIGMA_T, dev(lam), st)
    else:
        L.call("pk_fusion_terms_fwd", hm, off, var, tgt, w, gt, co, v["ws"], v["losses"], v["sigma"], B, K, H, W, x["input_size"][0],
               x["input_size"][1], lc.SIGMA_T, dev(lam), int(c.utw), st)
        L.call("pk_fusion_terms_bwd", hm, tgt, v["ws"], g3, None if gs is None else dev(gs), dev(g), v["d_hm"], v["d_off"], v["d_var"],
               v["d_coords"] if co is not None else None, B, K, H, W, lc.SIGMA_T, dev(lam), st)
    torch.cuda.synchronize()
    written = [k for k in sizes if k != "ws" and not (plain and k in ("sigma", "d_coords")) and not (k == "d_coords" and co is None)]
    return out, sizes, written


GUARD_CASES = [("13x11 K17", "random7+sigma", False), ("8x6 K5 coords", "random7+sigma", False), ("16x17 K12", "3total", True),
               ("8x6 K1 B257", "shape", False)]


@gpu
@pytest.mark.parametrize("name,upname,plain", GUARD_CASES, ids=lambda v: str(v))
def test_fusion_outputs_inside_guards_written_once_and_reproducible(ops, name, upname, plain):
    """outputs and a workspace of exactly PK_LOSS_WS_FLOATS(B, K) floats inside larger allocations: the guards keep their bits, every
    output element is written over its NaN, two launches give identical bytes; grad_total = 3 on the device scales every gradient"""
    hipops, L = ops
    c = next(c for c in lc.FUSION if c.name == name)
    up = next(u for u in lc.upstreams(c) if u[0] == upname)
    x = inputs(c)
    assert hipops.loss_ws_floats(c.B, c.K) == c.B * c.K * 24 + c.B * 16 * 4 + 16
    first, sizes, written = fusion_c_entries(L, c, x, up, plain)
    second, _, _ = fusion_c_entries(L, c, x, up, plain)
    for k, n in sizes.items():
        assert guards_hold(first[k][0], n) and guards_hold(second[k][0], n), f"{name}: wrote outside {k}"
    for k in written:
        assert not bool(torch.isnan(first[k][1]).any()), f"{name}: {k} has elements never written"
        assert torch.equal(first[k][0], second[k][0]), f"{name}: {k} differs between two launches"
    ref, o64, o32 = runs(c, up)
    scale = 1.0 if plain else 3.0              # pk_fusion_loss_bwd has no upstream vector: grad_total = 3 IS the 3 x total upstream
    shapes = dict(d_hm=ref["d_hm"].shape, d_off=ref["d_off"].shape, d_var=ref["d_var"].shape, d_coords=(c.B, c.K, 2), sigma=(c.B, c.K),
                  losses=(7,))
    names = ("d_hm", "d_off", "d_var", "d_coords")
    direct, sigma_share = None, dict.fromkeys(names, 0.0)
    if not plain:                               # loss_np with grad_total = 3; grad_sigma's share is not scaled by it
        direct = dict(zip(names, ln.fusion_backward(ref["state"], up[2], 3.0, up[3])))
        if up[3] is not None:
            sigma_share = dict(zip(names, ln.fusion_backward(ref["state"], np.zeros(7), None, up[3])))
    failures = []
    for k in written:
        got = host(first[k][1]).reshape(shapes[k])
        want, y32, y64 = ref[k], o32[k], o64[k]
        if k in names and direct is not None:   # the oracle's runs, scaled the same way, stay the yardstick
            want = direct[k]
            y32, y64 = (scale * (o[k] - sigma_share[k]) + sigma_share[k] for o in (o32, o64))
        ratio, at, ok = lc.judge(k, got, want, y32, y64, lc.tie_mask(ref["state"]) if k == "d_hm" else None)
        record(k, "C entry " + upname, ratio, c, at)
        if not ok:
            failures.append(f"{name} / {k}: {ratio:.3g} x yardstick at map {at}")
    assert not failures, "\n".join(failures)


# ================================================================================================ pixel loss
@gpu
@pytest.mark.parametrize("c", lc.PIXEL, ids=repr)
def test_pixel_loss_value_and_gradient(ops, c):
    hipops, L = ops
    pred, tgt, w = c.data()
    total = pred.size
    for kind in range(4):
        p, t, ww = dev(pred, True), dev(tgt), dev(w)
        loss = hipops.pixel_loss(p, t, ww, kind)
        loss.backward()
        ref, bound = ln.pixel_loss(pred, tgt, w, kind), lc.pixel_bound(total, ln.pixel_terms(pred, tgt, w, kind))
        err = abs(float(loss.detach()) - ref)
        record("pixel", f"kind {kind} value", err / bound, c, ())
        assert err <= bound, f"{c} kind {kind}: loss {float(loss.detach())!r}, reference {ref!r}, |error| / bound {err / bound:.3g}"
        dref, got = ln.pixel_loss_bwd(pred, tgt, w, kind), host(p.grad)
        rel = np.abs(got - dref) / np.where(dref == 0, 1.0, np.abs(dref))
        assert (got[dref == 0] == 0).all()
        at = np.unravel_index(np.argmax(rel), rel.shape)
        record("pixel", f"kind {kind} grad/4U", float(rel[at]) / (4 * lc.U), c, tuple(int(i) for i in at))
        assert rel[at] <= 4 * lc.U, f"{c} kind {kind}: d_pred{at} = {got[at]!r}, reference {dref[at]!r}, {rel[at] / lc.U:.3g} U"


@gpu
@pytest.mark.parametrize("name", ["HW 143", "backward wraps"])
def test_pixel_loss_inside_guards_and_reproducible(ops, name):
    """partial is exactly PK_REDUCE_BLOCKS floats; d_pred starts as NaN; guards keep their bits; two launches, identical bytes"""
    _, L = ops
    c = next(c for c in lc.PIXEL if c.name == name)
    pred, tgt, w = c.data()
    p, t, ww = dev(pred), dev(tgt), dev(w)
    bufs = []
    for _ in range(2):
        part, loss, dp = guarded(1024), guarded(1), guarded(pred.size)
        L.call("pk_pixel_loss_fwd", p, t, ww, part[1], loss[1], c.B, c.K, c.HW, 2, L.stream_ptr())
        L.call("pk_pixel_loss_bwd", p, t, ww, None, dp[1], c.B, c.K, c.HW, 2, L.stream_ptr())
        torch.cuda.synchronize()
        assert guards_hold(part[0], 1024) and guards_hold(loss[0], 1) and guards_hold(dp[0], pred.size)
        assert not bool(torch.isnan(dp[1]).any()) and not bool(torch.isnan(loss[1]).any())
        bufs.append((loss[0], dp[0]))
    assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][1], bufs[1][1])
    assert abs(float(bufs[0][0][GUARD:GUARD + 1].view(torch.float32)) - ln.pixel_loss(pred, tgt, w, 2)) <= lc.pixel_bound(
        pred.size, ln.pixel_terms(pred, tgt, w, 2))


# ================================================================================================ spatial statistics
@gpu
@pytest.mark.parametrize("c", lc.STATS, ids=repr)
def test_spatial_statistics_per_map(ops, c):
    hipops, L = ops
    hm, gm, gv = c.data()
    h = dev(hm, True)
    mean, var = hipops.spatial_stats(h)
    ((mean * dev(gm)).sum() + (var * dev(gv)).sum()).backward()
    ref = ln.spatial_stats(hm) + (ln.spatial_stats_bwd(hm, gm, gv),)
    o64, o32 = lc.stats_oracle(hm, gm, gv, torch.float64), lc.stats_oracle(hm, gm, gv, torch.float32)
    failures = []
    for i, (key, got) in enumerate((("mean", host(mean)), ("var", host(var)), ("d_stats", host(h.grad)))):
        assert not np.isnan(got).any()
        ratio, at, ok = lc.judge(key, got, ref[i], o32[i], o64[i])
        record(key, "spatial stats", ratio, c, at)
        if not ok:
            failures.append(f"{c} / {key}: {ratio:.3g} x yardstick at map {at}, bar {lc.M[key]}")
    assert not failures, "\n".join(failures)
    # the C entries into guarded outputs, twice
    BK, n = c.B * c.K, hm.size
    runs_ = []
    for _ in range(2):
        m, v, d = guarded(2 * BK), guarded(2 * BK), guarded(n)
        L.call("pk_spatial_stats", h.detach(), m[1], v[1], BK, c.H, c.W, L.stream_ptr())
        L.call("pk_spatial_stats_bwd", h.detach(), m[1], v[1], dev(gm), dev(gv), d[1], BK, c.H, c.W, L.stream_ptr())
        torch.cuda.synchronize()
        assert guards_hold(m[0], 2 * BK) and guards_hold(v[0], 2 * BK) and guards_hold(d[0], n)
        assert not any(bool(torch.isnan(b[1]).any()) for b in (m, v, d))
        runs_.append((m[0], v[0], d[0]))
    assert all(torch.equal(a, b) for a, b in zip(*runs_))
    assert torch.equal(runs_[0][2][GUARD:GUARD + n].view(torch.float32).view(h.shape), h.grad)
