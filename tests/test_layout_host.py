"""CPU tests of the layout unit's restatements (tests/layout_np.py) and of its host-side table builders: the bf16 reference on
hand-written bit patterns, the packing rules against a literal reading of the table, nnops._block_table, the offsets and views of
nnops.WeightCache._build, models.padded._box and the bookkeeping of padded._Table.  No test here needs a device."""
import numpy as np
import pytest
import torch

import layout_np as ln

PACK_CASES = [(0, 5, 3, 9), (0, 32, 32, 1), (0, 4, 11, 1), (1, 17, 12, 9), (1, 8, 8, 9), (1, 3, 5, 4), (2, 13, 78, 1), (2, 24, 24, 1)]


# ------------------------------------------------------------------------------------------------ the bf16 reference
def test_bf16_reference_rounds_to_nearest_even_on_hand_written_bits():
    got = ln.bf16_bits(ln.SPECIAL_F32.view(np.float32))
    for (f, b), g in zip(ln.SPECIALS, got):
        assert int(g) == b, f"float32 {f:#010x} -> bfloat16 {int(g):#06x}, expected {b:#06x}"
    # the list holds what the issue names: both kinds of tie, either side of a tie, both zeros, subnormals, the overflow, both infinities
    low = ln.SPECIAL_F32 & 0xFFFF
    tie = low == 0x8000
    assert (tie & ((ln.SPECIAL_F32 >> 16) & 1 == 0)).any() and (tie & ((ln.SPECIAL_F32 >> 16) & 1 == 1)).any()
    assert (low == 0x8001).any() and (low == 0x7FFF).any()
    assert {0x00000000, 0x80000000, 0x7F7FFFFF, 0x7F800000, 0xFF800000} <= set(int(v) for v in ln.SPECIAL_F32)
    expo = (ln.SPECIAL_F32 >> 23) & 0xFF
    assert ((expo == 0) & ((ln.SPECIAL_F32 & 0x7FFFFF) != 0)).sum() >= 4


def test_bf16_reference_against_integer_arithmetic():
    """round-to-nearest-even written with integers, on random bit patterns of every exponent (NaNs left out)"""
    rng = np.random.default_rng(1)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]
    want = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(ln.bf16_bits(u.view(np.float32)), want)


def test_plant_specials_places_every_value_and_keeps_the_ends():
    rng = np.random.default_rng(2)
    a = ln.normal_with_specials((7, 11, 3), rng)
    bits = a.reshape(-1).view(np.uint32)
    assert bits[0] == ln.SPECIAL_F32[0] and bits[-1] == ln.SPECIAL_F32[-1]
    assert set(int(v) for v in ln.SPECIAL_F32) <= set(int(v) for v in bits)
    assert int(np.isnan(a).sum()) == 1
    small = ln.normal_with_specials((5,), rng)
    assert small.reshape(-1).view(np.uint32)[0] == ln.SPECIAL_F32[0] and not np.isnan(small).any()


def test_assert_bits_reports_element_and_block_and_lets_nan_payloads_pass():
    ref = np.arange(3000, dtype=np.uint16)
    got = ref.copy()
    got[2050] ^= 1
    with pytest.raises(AssertionError, match=r"element 2050 \(block 2\)"):
        ln.assert_bits(got, ref, "x")
    ref[7], got[7], got[2050] = 0x7FC0, 0xFFC5, ref[2050]
    nan = np.zeros(3000, bool)
    nan[7] = True
    ln.assert_bits(got, ref, "x", nan)
    with pytest.raises(AssertionError, match="element 7 "):
        ln.assert_bits(got, ref, "x")
    got[7] = 0x7F80                       # an infinity is no NaN
    with pytest.raises(AssertionError, match="element 7 "):
        ln.assert_bits(got, ref, "x", nan)


# ------------------------------------------------------------------------------------------------ packing rules
@pytest.mark.parametrize("mode,N,C,T", PACK_CASES)
def test_pack_restatement_matches_the_rule_element_by_element(mode, N, C, T):
    rng = np.random.default_rng(10 * mode + N)
    w = rng.standard_normal((N, C, T)).astype(np.float32)
    Cp, Np = ln.up(C, 8), ln.up(N, 8)
    a, b = ln.pack_ref(w, N, C, T, mode, Cp, Np), ln.pack_ref_loops(w, N, C, T, mode, Cp, Np)
    assert a.shape == b.shape == ln.pack_shape(N, C, T, mode, Cp, Np)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pad = ln.pack_pad_mask(N, C, T, mode, Cp, Np)
    assert int(pad.sum()) == a.size - N * C * T and (a.view(np.uint32)[pad] == 0).all()
    assert np.array_equal(np.sort(a[~pad]), np.sort(w.reshape(-1)))              # a permutation of the source, nothing lost
    if mode == 1 and T > 1:
        assert not np.array_equal(a, ln.pack_ref(w[:, :, ::-1], N, C, T, mode, Cp, Np))      # the flip is visible


# ------------------------------------------------------------------------------------------------ block tables
def _nnops():
    from infantposeestimation_gaussianbias_amd import nnops
    return nnops


@pytest.mark.parametrize("sizes", [[0, 1, 1023, 1024, 1025], [1025, 0, 1024, 1, 1023, 0], [360, 1024, 3200, 2592, 576, 1248, 576], [1], [4096, 4097]])
def test_block_table_counts_first_blocks_and_total(sizes):
    blk_desc, blk_first, nb = _nnops()._block_table(sizes, 1024, "cpu")
    assert blk_desc.dtype == torch.int32 and blk_first.dtype == torch.int32
    want_desc, want_first, want_nb = ln.block_table_ref(sizes, 1024)
    assert nb == want_nb == sum((n + 1023) // 1024 for n in sizes)
    assert blk_desc.tolist() == want_desc and blk_first.tolist() == want_first
    counts = np.bincount(np.asarray(blk_desc.tolist(), np.int64), minlength=len(sizes))
    for i, n in enumerate(sizes):
        assert counts[i] == (0 if n == 0 else 1 if n <= 1024 else (n - 1) // 1024 + 1), (i, n)
    # every element of every descriptor is covered by exactly one workgroup: block b handles [1024 (b - first), +1024) of its descriptor
    for i, n in enumerate(sizes):
        seen = np.zeros(n, np.int32)
        for b in range(nb):
            if want_desc[b] == i:
                lo = 1024 * (b - blk_first[b].item())
                assert 0 <= lo < n
                seen[lo:lo + 1024] += 1
        assert (seen == 1).all()


def test_block_table_explicit_values():
    d, f, nb = _nnops()._block_table([0, 1, 1023, 1024, 1025], 1024, "cpu")
    assert nb == 5
    assert d.tolist() == [1, 2, 3, 4, 4]
    assert f.tolist() == [0, 1, 2, 3, 3]


# ------------------------------------------------------------------------------------------------ WeightCache._build
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c3 = torch.nn.Conv2d(3, 20, 3)
        self.c1 = torch.nn.Conv2d(20, 17, 1)
        self.fc = torch.nn.Linear(20, 52)
        self.shared = torch.nn.Conv2d(3, 20, 3)
        self.shared.weight = self.c3.weight


def test_weight_cache_build_offsets_aligned_disjoint_and_views():
    """_build runs on CPU tensors: the table rows, the 8-aligned disjoint regions, the block table and the dictionaries of views."""
    nnops = _nnops()
    net = _Net()
    wc = nnops.WeightCache(net)
    assert [tuple(e[1:]) for e in wc.entries] == [(20, 3, 9), (17, 20, 1), (52, 20, 1)]          # the shared weight once
    wc._build(torch.device("cpu"))
    desc = wc._desc.numpy().view(nnops._PACK_DTYPE)
    assert len(desc) == 6 and desc.dtype.itemsize == 48
    regions = []
    for k, (w, N, C, T) in enumerate(wc.entries):
        f, d = desc[2 * k], desc[2 * k + 1]
        Cp, Np = ln.up(C, 8), ln.up(N, 8)
        for row, mode, numel in ((f, 0, N * T * Cp), (d, 1 if T > 1 else 2, C * T * Np)):
            assert (row["src"], row["N"], row["C"], row["T"], row["mode"], row["Cp"], row["Np"], row["dst_numel"]) == \
                (w.data_ptr(), N, C, T, mode, Cp, Np, numel)
            assert row["dst_off"] % 8 == 0
            regions.append((int(row["dst_off"]), numel))
        assert wc.fwd[id(w)].shape == (N, T, Cp) and wc.dgrad[id(w)].shape == (C, T, Np)
        assert wc.fwd[id(w)].data_ptr() == wc.flat.data_ptr() + 2 * int(f["dst_off"])
        assert wc.dgrad[id(w)].data_ptr() == wc.flat.data_ptr() + 2 * int(d["dst_off"])
        assert wc.fwd[id(w)].is_contiguous() and wc.dgrad[id(w)].is_contiguous()
    assert set(wc.fwd) == set(wc.dgrad) == {id(e[0]) for e in wc.entries}
    regions.sort()
    for (o0, n0), (o1, _) in zip(regions, regions[1:]):
        assert o0 + n0 <= o1, "regions overlap"
        assert o1 == ln.up(o0 + n0, 8), "a region does not start at the next multiple of 8"
    assert regions[0][0] == 0 and wc.flat.numel() == ln.up(regions[-1][0] + regions[-1][1], 8) and wc.flat.dtype == torch.bfloat16
    want = ln.block_table_ref([int(r["dst_numel"]) for r in desc], 1024)
    assert (wc._blk_desc.tolist(), wc._blk_first.tolist(), wc._nb) == want


# ------------------------------------------------------------------------------------------------ padded._box, padded._Table
def _padded():
    from infantposeestimation_gaussianbias_amd.models import padded
    return padded


def test_box_head_structured_names():
    box = _padded()._box
    meta = {"stage2.0.branches.0.0": (2, 39, 40)}
    E = torch.empty
    pre = "stage2.0.branches.0.0.attn."
    assert box(pre + "qkv.weight", E(234, 78), E(240, 80), meta) == ([3, 2, 39, 78], [3, 2, 40, 80])
    assert box(pre + "qkv.bias", E(234), E(240), meta) == ([1, 3, 2, 39], [1, 3, 2, 40])
    assert box(pre + "proj.weight", E(78, 78), E(80, 80), meta) == ([1, 78, 2, 39], [1, 80, 2, 40])
    # plain members of an attention module, and attention weights of a block that is not in the table, are zero-extended
    assert box(pre + "proj.bias", E(78), E(80), meta) == ([1, 1, 1, 78], [1, 1, 1, 80])
    assert box(pre + "relative_position_bias_table", E(169, 2), E(169, 2), meta) == ([1, 1, 169, 2], [1, 1, 169, 2])
    assert box("other.attn.qkv.weight", E(234, 78), E(240, 80), meta) == ([1, 1, 234, 78], [1, 1, 240, 80])
    # an unpadded block keeps the plain form
    assert box(pre + "qkv.weight", E(240, 80), E(240, 80), {"stage2.0.branches.0.0": (2, 40, 40)}) == ([1, 1, 240, 80], [1, 1, 240, 80])


def test_box_plain_ranks_and_refusals():
    box = _padded()._box
    E = torch.empty
    assert box("a", E(()), E(()), {}) == ([1, 1, 1, 1], [1, 1, 1, 1])
    assert box("a", E(78), E(80), {}) == ([1, 1, 1, 78], [1, 1, 1, 80])
    assert box("a", E(156, 78), E(160, 80), {}) == ([1, 1, 156, 78], [1, 1, 160, 80])
    assert box("a", E(5, 156, 78), E(5, 160, 80), {}) == ([1, 5, 156, 78], [1, 5, 160, 80])
    assert box("a", E(18, 18, 3, 3), E(24, 24, 3, 3), {}) == ([18, 18, 3, 3], [24, 24, 3, 3])
    with pytest.raises(ValueError, match="rank 5"):
        box("a", E(2, 2, 2, 2, 2), E(2, 2, 2, 2, 2), {})
    with pytest.raises(ValueError, match="does not fit"):
        box("a", E(18, 25, 3, 3), E(24, 24, 3, 3), {})
    with pytest.raises(ValueError, match="does not fit"):
        box("a", E(81), E(80), {})


def test_embed_table_rows_and_blocks():
    padded = _padded()
    rows = [(1000, 0, [1, 1, 1, 78], [1, 1, 1, 80]), (2000, 80, [1, 1, 156, 78], [1, 1, 160, 80]), (3000, 12880, [1, 1, 1, 1], [1, 1, 1, 1]),
            (4000, 12884, [1, 1, 32, 64], [1, 1, 32, 64])]
    t = padded._Table(rows, "cpu")
    desc = t.desc.numpy().view(padded._EMBED_DTYPE)
    assert desc.dtype.itemsize == 56
    assert desc["real"].tolist() == [1000, 2000, 3000, 4000] and desc["off"].tolist() == [0, 80, 12880, 12884]
    assert desc["numel"].tolist() == [78, 12168, 1, 2048]
    assert desc["r"].tolist() == [r[2] for r in rows] and desc["p"].tolist() == [r[3] for r in rows]
    want = ln.block_table_ref([78, 12168, 1, 2048], 1024)
    assert (t.blk_desc.tolist(), t.blk_first.tolist(), t.nb) == want and t.nb == 1 + 12 + 1 + 2
    assert padded._Table([], "cpu").n == 0


def test_embed_by_name_is_a_zero_extension_of_every_head():
    rng = np.random.default_rng(3)
    pre = "b.attn."
    w = rng.standard_normal((234, 78)).astype(np.float32)
    tw, m = ln.embed_by_name(pre + "qkv.weight", w, (240, 80), heads=2)
    assert int(m.sum()) == w.size and np.array_equal(tw[m], w.reshape(-1)) and (tw[~m] == 0).all()
    # q of head 1, real row 39 + 5 -> twin row 40 + 5; v of head 0, real row 156 + 38 -> twin row 160 + 38; rows 39 and 79 of each part are padding
    assert np.array_equal(tw[45, :78], w[44]) and np.array_equal(tw[198, :78], w[194])
    assert not tw[39].any() and not tw[79].any() and not tw[:, 78:].any()
    b = rng.standard_normal(234).astype(np.float32)
    tb, m = ln.embed_by_name(pre + "qkv.bias", b, (240,), heads=2)
    assert tb[45] == b[44] and tb[39] == 0 and int(m.sum()) == 234
    p = rng.standard_normal((78, 78)).astype(np.float32)
    tp, m = ln.embed_by_name(pre + "proj.weight", p, (80, 80), heads=2)
    assert np.array_equal(tp[:78, 40:79], p[:, 39:]) and not tp[:, 39].any() and not tp[78:].any() and int(m.sum()) == p.size
    # the same placement read through the box form of the kernel
    padded = _padded()
    for name, real, twin in ((pre + "qkv.weight", w, tw), (pre + "qkv.bias", b, tb), (pre + "proj.weight", p, tp)):
        r, pp = padded._box(name, torch.from_numpy(real), torch.from_numpy(twin), {"b": (2, 39, 40)})
        assert np.array_equal(ln.box_view(twin.reshape(-1), 0, r, pp).reshape(-1), real.reshape(-1))


# ------------------------------------------------------------------------------------------------ the other restatements
def test_row_move_and_drop_path_restatements():
    rng = np.random.default_rng(4)
    src = rng.integers(1, 2 ** 32, (6, 3), dtype=np.uint64).astype(np.uint32)
    m = np.array([4, -1, 0, 4, 5], np.int32)
    g = ln.rows_gather_ref(src, m)
    assert np.array_equal(g[0], src[4]) and not g[1].any() and np.array_equal(g[3], src[4]) and g.shape == (5, 3)
    dst = np.full((7, 3), ln.F32_SENTINEL, np.uint32)
    s = ln.rows_scatter_ref(src[:5], np.array([6, -1, 2, 0, -1], np.int32), dst)
    assert np.array_equal(s[6], src[0]) and np.array_equal(s[2], src[2]) and np.array_equal(s[0], src[3])
    assert (s[[1, 3, 4, 5]] == ln.F32_SENTINEL).all() and (dst == ln.F32_SENTINEL).all()
    x = rng.standard_normal((3, 5)).astype(np.float32)
    y = ln.drop_path_ref(x, np.array([1, 0, 1], np.float32), 0.75)
    assert y.dtype == np.float32 and np.array_equal(y[0], x[0] / np.float32(0.75)) and not y[1].any()


def test_softplus_window_restatement():
    """neighbours and boundary distances on hand-made values; the share of a normal sample inside the window is far below the bar"""
    lo, hi, dist = ln.bf16_neighbours(np.array([1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.5 + 2.0 ** -9), 1.0 + 2.0 ** -12, 0.3]))
    assert lo[0] == 1.0 and hi[0] == 1.0 + 2.0 ** -7 and dist[0] == 2.0 ** -20           # the boundary is 1 + 2^-8
    assert lo[1] == -1.5 and hi[1] == -(1.5 + 2.0 ** -7) and dist[1] == 2.0 ** -9        # boundaries at 1.5 -+ 2^-8
    assert dist[2] == 2.0 ** -9 + 2.0 ** -12                      # just above a power of two: the nearest boundary is 1 - 2^-9, below it
    assert lo[3] <= 0.3 <= hi[3] and hi[3] - lo[3] == 2.0 ** -9
    rng = np.random.default_rng(5)
    x = rng.standard_normal(400000).astype(np.float32)
    z = np.maximum(1.5 * rng.standard_normal(400000), -3.0)
    sp = np.log1p(np.exp(z)).astype(np.float32)
    assert (1.0 - np.exp(-sp.astype(np.float64))).min() >= 0.047
    rne, lo_b, hi_b, inside = ln.softplus_window(x, sp)
    share = inside.mean()
    assert share <= 0.005 and share > 0, share
    assert ((rne == lo_b) | (rne == hi_b)).all()
    # an fp32 evaluation of the same expression disagrees with RNE(r) only inside the window
    r32 = x * (np.float32(1.0) - np.exp(-sp).astype(np.float32))
    bad = ln.bf16_bits(r32) != rne
    assert not (bad & ~inside).any()
    assert ((ln.bf16_bits(r32) == lo_b) | (ln.bf16_bits(r32) == hi_b)).all()
