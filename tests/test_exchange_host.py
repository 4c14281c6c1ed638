"""Exchange unit, host side: the gather window of the up-sampling backward against the taps for every integer ratio up to 200, the numpy
restatement (tests/exchange_np.py) against F.interpolate, the case tables of the device tests against the launch arithmetic, and
the proof that the device tests' bounds can fail: a reference with one contributor dropped violates them.  Nothing here launches a
kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exchange_cases as xc
import exchange_np as xn

N_MAX = 200


def test_gather_window_covers_every_contributor_of_an_integer_ratio():
    """Every output row with a non-zero weight on source row ys lies inside gather_window(ys, H, Hs) wherever H is a multiple of Hs,
    H <= 200 (the same expression serves columns), and the window stays inside [0, H]: the kernel reads dy at every row it scans.
    Ratios that are not integers are the KNOWN GAP of gather_window's docstring: the same check fails for 16 447 of the 20 100 pairs
    (13 <- 12 and 65 <- 9 among them), which is why this test does not ask for them yet."""
    for Hs in range(1, N_MAX + 1):
        for H in range(Hs, N_MAX + 1, Hs):
            first, last = xn.support(H, Hs)
            assert (first <= last).all(), (H, Hs)                  # every source row has a contributor
            assert xn.window_covers(H, Hs), (H, Hs)
    for H, Hs in ((1, 1), (13, 12), (65, 9), (200, 199), (200, 7), (64, 8)):
        lo, hi = xn.gather_window(np.arange(Hs), H, Hs)
        assert (lo >= 0).all() and (hi <= H).all()


def test_the_exact_even_window_is_exact():
    """For an exact even ratio r the window IS the support: 2r rows, clipped at the borders, also where 1 / r is not a float32."""
    for Hs in (1, 2, 3, 7, 16):
        for r in (2, 4, 6, 8, 10, 12):
            first, last = xn.support(Hs * r, Hs)
            lo, hi = xn.gather_window(np.arange(Hs), Hs * r, Hs)
            assert (first == lo).all() and (last == hi - 1).all(), (Hs, r)


# ------------------------------------------------------------------------------------------------ the restatement vs F.interpolate
ODD_SIZES = [((5, 4), (9, 7)), ((12, 12), (13, 13)), ((9, 7), (65, 49)), ((3, 5), (11, 200)), ((17, 13), (17, 49)), ((1, 1), (4, 3))]


@pytest.mark.parametrize("src,dst", ODD_SIZES)
def test_reference_agrees_with_interpolate(src, dst):
    """fuse_sum_ref's up-sampling is F.interpolate(mode='bilinear', align_corners=False) in float64, but for the scale: the kernels form
    n_in / n_out and the source coordinate in float32.  A coordinate below 200 carries an absolute error of at most 3 roundings of 2^-24
    relative on values below 200 (the quotient, the product, the difference): 3 x 200 x 2^-24 < 3.6e-5 per axis, which moves the weights
    by as much; the output moves by at most that times the difference of neighbouring values, per axis.  The data is N(0, 1), clipped to
    |v| <= 4: neighbours differ by at most 8, so 2 x 8 x 3.6e-5 = 5.8e-4 bounds the difference.  Measured: at most 3.3e-6 over these sizes.
    The transpose (upsample_bwd_ref) is held against autograd the same way: a source pixel collects at most
    (2 x 200/5 + 2) x (2 x 11/3 + 2) < 800 taps, each weight wy wx moves by at most 2 x 3.6e-5 and meets |g| <= 4: 800 x 4 x 7.2e-5 = 0.23,
    a worst case that no data reaches; measured: at most 8.9e-6."""
    rng = np.random.default_rng(sum(src) + 7 * sum(dst))
    x = np.clip(rng.standard_normal((2, src[0], src[1], 8)), -4, 4)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt = F.interpolate(xt, size=list(dst), mode="bilinear", align_corners=False)
    ours = xn.fuse_sum_ref([x], dst[0], dst[1], relu=0)
    d = np.abs(ours - yt.detach().permute(0, 2, 3, 1).numpy()).max()
    g = np.clip(rng.standard_normal((2, dst[0], dst[1], 8)), -4, 4)
    yt.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    db = np.abs(xn.upsample_bwd_ref(g, src[0], src[1]) - xt.grad.permute(0, 2, 3, 1).numpy()).max()
    print(f"{src} -> {dst}: forward differs by {d:.3g}, backward by {db:.3g}")
    assert d <= 5.8e-4
    assert db <= 0.23


def test_backward_reference_is_the_transpose_of_the_forward():
    """<up(x), g> == <x, up^T(g)> in float64 (up to the float32 sum of two clamped-together taps, 2^-24 relative), mask included."""
    rng = np.random.default_rng(3)
    for (hs, ws), (h, w) in ODD_SIZES:
        x, g = rng.standard_normal((2, hs, ws, 8)), rng.standard_normal((2, h, w, 8))
        lhs = (xn.fuse_sum_ref([x], h, w, relu=0) * g).sum()
        rhs = (x * xn.upsample_bwd_ref(g, hs, ws)).sum()
        scale = (np.abs(xn.fuse_sum_ref([np.abs(x)], h, w, relu=0)) * np.abs(g)).sum()
        assert abs(lhs - rhs) <= 2.0 ** -22 * scale, ((hs, ws), (h, w))
    g, m = rng.standard_normal((1, 9, 7, 8)), xc.mask_values((1, 9, 7, 8), rng)
    assert np.array_equal(xn.upsample_bwd_ref(g, 5, 4, m), xn.upsample_bwd_ref(np.where(m > 0, g, 0), 5, 4))
    assert (m == 0).any() and np.signbit(m[m == 0]).any() and (m < 0).any()


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_tables_reach_the_plans_they_name():
    caps = (xn.CHUNK_GRID_CAP, xn.CHUNK_GRID_CAP_GROUPED)
    for c in xc.FUSE + xc.FUSE_MASKED + [xc.FUSE_WRAP, xc.FUSE_WRAP_GROUPED]:
        assert c.C % 8 == 0 and 1 <= len(c.sizes) <= 4 and all(h <= c.H and w <= c.W for h, w in c.sizes)
        for declared, cap in zip((c.single, c.grouped), caps):
            if declared is not None:
                assert xn.fuse_plan(c.B, c.H, c.W, c.C, cap)[1:] == declared, (c.name, cap)
    chunks = xn.fuse_plan(1, 65, 63, 2056, xn.CHUNK_GRID_CAP)[0]
    assert 0 < chunks - 4096 * 256 < 4096 and chunks < 1 << 24 and xc.FUSE_WRAP.C // 8 == 257
    chunks = xn.fuse_plan(1, 65, 63, 1032, xn.CHUNK_GRID_CAP_GROUPED)[0]
    assert 0 < chunks - 2048 * 256 < 4096
    assert {len(c.sizes) for c in xc.FUSE} == {1, 2, 3, 4} and {c.relu for c in xc.FUSE} == {0, 1} and {c.C for c in xc.FUSE} == {8, 24}
    assert any(xn.fuse_plan(c.B, c.H, c.W, c.C, 4096)[0] % 256 for c in xc.FUSE)
    assert len(xc.FUSE) <= xn.GROUP_MAX and len(xc.FUSE_WRAP_GROUP) <= xn.GROUP_MAX
    for c in xc.UP + xc.UP_PARTIAL:
        assert c.C % 8 == 0 and c.Hs <= c.H and c.Ws <= c.W
        for declared, cap in zip((c.single, c.grouped), caps):
            chunks, split, blocks, trips, last = xn.upsample_plan(c.B, c.H, c.Hs, c.Ws, c.C, cap)
            assert (split, (blocks, trips)) == (c.split, declared), (c.name, cap, split, blocks, trips)
        if c.name in xc.LAST_TRIP:
            assert last == xc.LAST_TRIP[c.name] and last * c.split % 64 != 0          # the last trip ends inside a wavefront
    for split in (1, 4, 16):
        assert any(c.split == split and c.positive and (c.H % c.Hs or c.W % c.Ws) for c in xc.UP), split             # a ratio that is no integer
        assert any(c.split == split and c.H == c.Hs * {1: 2, 4: 4, 16: 8}[split] for c in xc.UP), split        # exact ratio 2 / 4 / 8
    # every case stays where the kernel's window contains all contributors (gather_window: KNOWN GAP)
    for c in xc.UP + xc.UP_PARTIAL:
        assert xn.window_covers(c.H, c.Hs) and xn.window_covers(c.W, c.Ws), c.name


# ------------------------------------------------------------------------------------------------ the bounds can fail
@pytest.mark.parametrize("c", xc.UP, ids=lambda c: c.name)
def test_backward_bound_notices_one_dropped_tap(c):
    """At sampled elements (the first and the last among them) the scatter is written out tap by tap: its sum is the matrix-form
    reference, and without its largest single term it violates the bound of that element, mask present and absent."""
    dy, mask = c.data()
    for m in (None, mask):
        ref, bnd = c.reference(dy, m)
        for b, ys, xs, ch in xc.sample_elements(ref.shape, c.seed):
            terms = xc.up_contributions(c, dy, m, b, ys, xs, ch)
            r = ref[b, ys, xs, ch]
            assert abs(terms.sum() - r) <= 1e-12 * np.abs(terms).sum() + 1e-300
            if not np.abs(terms).max() > 0:
                assert m is not None                       # every contributor masked
                continue
            assert np.abs(terms).max() > bnd[b, ys, xs, ch], (c.name, (b, ys, xs, ch), np.abs(terms).max(), bnd[b, ys, xs, ch])


def test_gather_window_reproduces_the_reference_on_every_case():
    for c in xc.UP:
        dy, mask = c.data()
        assert np.array_equal(xn.upsample_bwd_windowed(dy, c.Hs, c.Ws, xn.gather_window, mask), xn.upsample_bwd_ref(dy, c.Hs, c.Ws, mask)), c.name


@pytest.mark.parametrize("c", xc.FUSE + xc.FUSE_MASKED, ids=lambda c: c.name)
def test_fused_sum_bound_notices_one_dropped_term(c):
    """At sampled elements the sum is written out product by product: it is the reference, and without its largest product it violates
    the bound of that element (where the ReLU does not hide both)."""
    ins, mask = c.data()
    ref, bnd = c.reference(ins, mask)
    seen = 0
    for b, y, x, ch in xc.sample_elements(ref.shape, c.seed):
        terms = np.array(xc.fuse_contributions(c, ins, mask, b, y, x, ch))
        total = terms.sum()
        want = max(total, 0) if c.relu else total
        assert abs(want - ref[b, y, x, ch]) <= 1e-12 * np.abs(terms).sum()
        dropped = total - terms[np.argmax(np.abs(terms))]
        dropped = max(dropped, 0) if c.relu else dropped
        if (c.relu and total <= 0 and dropped <= 0) or not np.abs(terms).max() > 0:
            continue
        seen += 1
        assert abs(dropped - ref[b, y, x, ch]) > bnd[b, y, x, ch], (c.name, (b, y, x, ch))
    assert seen >= 1
