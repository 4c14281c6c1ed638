"""Every kernel of csrc/pk_exchange.hip (pk_fuse_sum, pk_fuse_sum_group, pk_upsample_bilinear_bwd, pk_upsample_bwd_group) per element against
float64, at the smallest shapes that reach each path: one to four terms, same-size terms only, ratios 2 / 4 / 8, odd targets, ReLU on
and off, one channel chunk per pixel and three, chunk counts that are no multiple of 256, a grid-stride loop that takes a second, partly
empty trip (single launch: past 4096 x 256 chunks; group member: past 2048 x 256, between one-chunk members), the masked term of the
group form and its refusal; for the backward 1 / 4 / 16 lanes per chunk on exact even ratios (the 2r-row window) and on ratios that are
not integers (the generic window), ratio 1 and 3, a last trip that ends inside a wavefront, the mask present and absent, members of
different lane counts in one launch, and two launches of a wrapped 16-lane case byte for byte.

The cases, their declared plans, the inputs (seeded, bf16 values; strictly positive gradients where a missing tap must not cancel) and
the bound are tests/exchange_cases.py's; its docstring derives the bound:  |got - ref| <= 2^-8 |ref| + (1 + 2^-8) k 2^-24 mag  per element,
k = 5 + n for the sum of n terms, k = n + 7 for a backward element with n contributors, mag the sum of the magnitudes of the products.
The references are tests/exchange_np.py's (float64, weights from the float32 taps, the backward over ALL output pixels, no window);
tests/test_exchange_host.py ties them to F.interpolate and shows that one dropped contributor violates the bound in every case.
Entries are called through the C-ABI.  The module prints the worst |error| / bound of each family at its end.

Guards: every input is a view between 4096 NaN elements on either side; outputs start as NaN (every element must be written) and
are followed, inside the same allocation, by 4096 sentinel elements that must stay.

Not covered: ratios whose contributors the generic gather window does not contain -- most ratios that are not integers, 13 <- 12 and
65 <- 9 among them (KNOWN GAP in exchange_np.gather_window's docstring: the kernel leaves such contributors out); the backward cases here
keep to sizes where it contains them, and the host test holds the tables to that.  2^24 chunks and more (the exact-division branch of the index split) need tensors of 268 MB and up; no configuration
reaches it.  The single-launch backward is not wrapped (4096 x 256 / 16 chunks at ratio 8 means a 17 M-element gradient); the same body
wraps here as a group member."""
import numpy as np
import pytest
import torch

import exchange_cases as xc
import exchange_np as xn

gpu = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
GUARD = 4096
SENT = 24576.0            # exact in bf16
WORST = {}                # family -> (largest |error| / bound, where)
ERR_INVALID = -1
REFS = {}                 # case name -> (inputs, mask, reference, bound): computed once, never changed


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    yield _lib
    print()
    for fam, (ratio, what) in sorted(WORST.items()):
        print(f"{fam}: worst |error| / bound {ratio:.3g} ({what})")


def case_data(c):
    if c.name not in REFS:
        if isinstance(c, xc.Fuse):
            ins, mask = c.data()
            REFS[c.name] = (ins, mask) + c.reference(ins, mask)
        else:
            dy, mask = c.data()
            REFS[c.name] = (dy, mask) + c.reference(dy, None) + c.reference(dy, mask)
        for a in REFS[c.name]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return REFS[c.name]


def to_dev(a):
    """numpy float32 of bf16 values -> bf16 device view between NaN guards (the buffer stays alive through the view)"""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=BF, device=DEV)
    view = buf[GUARD:GUARD + a.size].view(a.shape)
    host = torch.from_numpy(a.copy())
    view.copy_(host)
    assert view.data_ptr() % 16 == 0
    assert torch.equal(view.float().cpu(), host)          # the values are bf16 values: nothing was rounded
    return view


def new_out(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), dtype=BF, device=DEV)
    buf[n:] = SENT
    return buf, buf[:n].view(shape)


def hold(family, name, out, ref, bnd):
    buf, view = out
    got = view.float().cpu().numpy().astype(np.float64)
    assert bool((buf[view.numel():] == SENT).all()), f"{name}: wrote past the end of the output"
    unwritten = np.isnan(got)
    assert not unwritten.any(), f"{name}: {int(unwritten.sum())} elements never written, first at {np.argwhere(unwritten)[0]}"
    err = np.abs(got - ref)
    exact = bnd == 0
    assert (err[exact] == 0).all(), f"{name}: a sum of zeros is not zero"
    ratio = np.where(exact, 0.0, err / np.where(exact, 1.0, bnd))
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    w = float(ratio[at])
    print(f"{family} / {name}: worst |error| / bound {w:.3g} at {tuple(int(i) for i in at)} (got {got[at]:.6g}, reference {ref[at]:.6g})")
    if w > WORST.get(family, (0.0, ""))[0]:
        WORST[family] = (w, name)
    assert w <= 1.0, (f"{name}: |error| / bound {w:.3g} at {tuple(int(i) for i in at)}: got {float(got[at])!r}, reference {float(ref[at])!r}, "
                      f"bound {float(bnd[at])!r}; {int((ratio > 1).sum())} of {ratio.size} elements over")


def stream():
    return torch.cuda.current_stream().cuda_stream


def desc_types():
    from infantposeestimation_gaussianbias_amd import exchange          # the host layouts, held against the library's sizeof at import
    return exchange.FUSE_DT, exchange.UPB_DT


def fuse_desc(c, ins, mask, out_view):
    d = np.zeros(1, dtype=desc_types()[0])[0]
    n = len(ins)
    d["inputs"] = [t.data_ptr() for t in ins] + [0] * (4 - n)
    d["in_h"] = [t.shape[1] for t in ins] + [0] * (4 - n)
    d["in_w"] = [t.shape[2] for t in ins] + [0] * (4 - n)
    d["n_inputs"], d["out"], d["mask_y"] = n, out_view.data_ptr(), 0 if mask is None else mask.data_ptr()
    d["B"], d["H"], d["W"], d["C"], d["relu"] = c.B, c.H, c.W, c.C, c.relu
    return d


def up_desc(c, dy, mask, out_view):
    d = np.zeros(1, dtype=desc_types()[1])[0]
    d["dy"], d["mask_y"], d["dsrc"] = dy.data_ptr(), 0 if mask is None else mask.data_ptr(), out_view.data_ptr()
    d["B"], d["H"], d["W"], d["Hs"], d["Ws"], d["C"] = c.B, c.H, c.W, c.Hs, c.Ws, c.C
    return d


def launch_group(L, entry, rows):
    arr = np.zeros(len(rows), dtype=rows[0].dtype)
    for i, r in enumerate(rows):
        arr[i] = r
    rc = getattr(L.lib, entry)(arr.ctypes.data, len(rows), stream())
    torch.cuda.synchronize()
    return rc


# ================================================================================================ fused sum
@gpu
@pytest.mark.parametrize("c", xc.FUSE + [xc.FUSE_WRAP], ids=lambda c: c.name)
def test_fuse_sum(L, c):
    assert xn.fuse_plan(c.B, c.H, c.W, c.C, xn.CHUNK_GRID_CAP)[1:] == c.single
    ins, _, ref, bnd = case_data(c)
    dev = [to_dev(t) for t in ins]
    out = new_out(ref.shape)
    ptrs = np.array([t.data_ptr() for t in dev], np.uint64)
    hs, ws = np.array([t.shape[1] for t in dev], np.int32), np.array([t.shape[2] for t in dev], np.int32)
    rc = L.lib.pk_fuse_sum(ptrs.ctypes.data, hs.ctypes.data, ws.ctypes.data, len(dev), out[1].data_ptr(), c.B, c.H, c.W, c.C, c.relu, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.lib.pk_last_error_string()
    hold("fused sum, single launch", c.name, out, ref, bnd)


def run_fuse_group(L, members, family):
    rows, outs, keep = [], [], []
    for c in members:
        assert xn.fuse_plan(c.B, c.H, c.W, c.C, xn.CHUNK_GRID_CAP_GROUPED)[1:] == c.grouped
        ins, mask, ref, bnd = case_data(c)
        dev, dm = [to_dev(t) for t in ins], (None if mask is None else to_dev(mask))
        out = new_out(ref.shape)
        rows.append(fuse_desc(c, dev, dm, out[1]))
        outs.append((c, out, ref, bnd))
        keep.append((dev, dm))
    rc = launch_group(L, "pk_fuse_sum_group", rows)
    assert rc == 0, L.lib.pk_last_error_string()
    for i, (c, out, ref, bnd) in enumerate(outs):
        hold(family, f"member {i}: {c.name}", out, ref, bnd)


@gpu
def test_fuse_sum_group(L):
    """every small case as a member of ONE launch"""
    run_fuse_group(L, xc.FUSE, "fused sum, group")


@gpu
def test_fuse_sum_group_wrapped_member_between_small_ones(L):
    """a member whose 2048 workgroups take a second trip, one-chunk members on either side of it: the member search at its boundaries"""
    run_fuse_group(L, xc.FUSE_WRAP_GROUP, "fused sum, group")


@gpu
def test_fuse_sum_group_masked_term(L):
    """term 0 counts only where mask_y > 0: zeros, -0.0 and negatives do not pass; the other terms are not masked"""
    for c in xc.FUSE_MASKED:
        mask = case_data(c)[1]
        assert (mask == 0).any() and np.signbit(mask[mask == 0]).any() and (mask < 0).any() and (mask > 0).any()
    run_fuse_group(L, xc.FUSE_MASKED, "fused sum, masked")


@gpu
def test_fuse_sum_group_refuses_a_small_masked_term(L):
    """mask_y with a term 0 smaller than the output: PK_ERR_INVALID for the whole group, nothing launched, no output touched"""
    good, bad = xc.FUSE_MASKED[1], xc.Fuse("refused", 1, 9, 7, 8, [(5, 4), (9, 7)], 0, None, None, mask=True, seed=33)
    rows, outs, keep = [], [], []
    for c in (good, bad):
        ins, mask = c.data()
        dev, dm = [to_dev(t) for t in ins], to_dev(mask)
        buf = torch.full((c.B * c.H * c.W * c.C + GUARD,), SENT, dtype=BF, device=DEV)
        rows.append(fuse_desc(c, dev, dm, buf))
        outs.append(buf)
        keep.append((dev, dm))
    rc = launch_group(L, "pk_fuse_sum_group", rows)
    assert rc == ERR_INVALID and b"masked term" in L.lib.pk_last_error_string()
    for buf in outs:
        assert bool((buf == SENT).all())
    assert launch_group(L, "pk_fuse_sum_group", rows[:1]) == 0          # the good member alone is accepted


# ================================================================================================ up-sampling backward
@gpu
@pytest.mark.parametrize("c", xc.UP, ids=lambda c: c.name)
def test_upsample_bwd(L, c):
    assert xn.upsample_plan(c.B, c.H, c.Hs, c.Ws, c.C, xn.CHUNK_GRID_CAP)[1:4] == (c.split,) + c.single
    dy, _, ref, bnd, _, _ = case_data(c)
    d = to_dev(dy)
    out = new_out(ref.shape)
    rc = L.lib.pk_upsample_bilinear_bwd(d.data_ptr(), out[1].data_ptr(), c.B, c.H, c.W, c.Hs, c.Ws, c.C, stream())
    torch.cuda.synchronize()
    assert rc == 0, L.lib.pk_last_error_string()
    hold(f"backward, single launch, {c.split} lanes", c.name, out, ref, bnd)


def run_up_group(L, members):
    """members: [(case, masked)] -> the raw bytes of every output"""
    rows, outs, keep = [], [], []
    for c, masked in members:
        assert xn.upsample_plan(c.B, c.H, c.Hs, c.Ws, c.C, xn.CHUNK_GRID_CAP_GROUPED)[1:4] == (c.split,) + c.grouped
        dy, mask, ref, bnd, mref, mbnd = case_data(c)
        d, dm = to_dev(dy), (to_dev(mask) if masked else None)
        out = new_out(ref.shape)
        rows.append(up_desc(c, d, dm, out[1]))
        outs.append((c, masked, out, mref if masked else ref, mbnd if masked else bnd))
        keep.append((d, dm))
    rc = launch_group(L, "pk_upsample_bwd_group", rows)
    assert rc == 0, L.lib.pk_last_error_string()
    raw = [out[0].view(torch.int16).cpu() for _, _, out, _, _ in outs]
    for i, (c, masked, out, ref, bnd) in enumerate(outs):
        hold(f"backward, group, {c.split} lanes", f"member {i}: {c.name}{', masked' if masked else ''}", out, ref, bnd)
    return raw


UP_GROUPS = [[(c, i % 2 == k) for i, c in enumerate(xc.UP[s:s + xn.GROUP_MAX])] for s in range(0, len(xc.UP), xn.GROUP_MAX) for k in (0, 1)]


@gpu
@pytest.mark.parametrize("members", UP_GROUPS, ids=lambda m: f"{m[0][0].name} on, {'masked' if m[0][1] else 'plain'} first")
def test_upsample_bwd_group(L, members):
    """every small case as a group member, with the mask and without it; members of different lane counts share each launch"""
    assert len({c.split for c, _ in members}) >= 2
    run_up_group(L, members)


@gpu
@pytest.mark.parametrize("c", xc.UP_PARTIAL, ids=lambda c: c.name)
def test_upsample_bwd_group_partial_last_trip(L, c):
    """2048 workgroups, a second trip in which only a few chunks are on and the last of them end inside a wavefront: every lane still
    reaches the lane sums (a uniform trip count), lanes that are off store nothing.  Between members with one and with other lane
    counts; launched twice: identical bytes (the butterfly's order is fixed)."""
    chunks, split, blocks, trips, last = xn.upsample_plan(c.B, c.H, c.Hs, c.Ws, c.C, xn.CHUNK_GRID_CAP_GROUPED)
    assert (split, blocks, trips, last) == (c.split, 2048, 2, xc.LAST_TRIP[c.name])
    members = [(xc.UP[0], False), (c, c.split == 16), (xc.UP[1] if c.split == 16 else xc.UP[2], True)]
    first = run_up_group(L, members)
    second = run_up_group(L, members)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
