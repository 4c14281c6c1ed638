"""Every entry of csrc/pk_layout.hip (pk_pack_weights, pk_embed_boxes, pk_nchw_f32_to_nhwc_bf16, pk_rows_by_map, pk_drop_path_f32) and
the two host classes that build their tables (nnops.WeightCache, models.padded.PaddedTwin) bit for bit against tests/layout_np.py, at
the smallest sizes that reach each regime: a partial block, exactly one block, several blocks and a partial one, descriptors whose
table order differs from the order of their destinations, padded and unpadded lanes, head-structured boxes, and row moves, DropPath and
the layout conversion past 4096 x 256 elements, where the grid-stride loop takes a second, partly empty trip.

Conventions: every destination holds a sentinel before a launch (bf16 0x7FC1, fp32 0x7FC00123, both NaNs no copy or conversion of a
planted value produces); "written" means the sentinel is gone, "untouched" that its bits are still there; comparisons are equalities
of bits through integer views, except that a NaN source need only give a NaN.  Sources are normal samples with the hand-written
special values of layout_np.SPECIALS (ties, the neighbours of ties, both zeros, subnormals, the overflow to inf, both infinities) at
the first, the last and some interior elements.  Destinations of scattering kernels lie inside a larger allocation, with sentinel
elements in front and behind that must stay.

The one bar that is not an equality is the softplus-derivative path of the layout conversion (hardware exponential):
layout_np.softplus_window states it; the test prints the share of elements near a rounding boundary and the number of mismatches."""
import numpy as np
import pytest
import torch

import layout_np as ln
from recipe import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096


@pytest.fixture(scope="module")
def L():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent16(n):
    """n bf16 elements holding the sentinel"""
    return torch.full((n,), ln.BF16_SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def sent32(n):
    return torch.full((n,), ln.F32_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    """device or host tensor -> numpy unsigned view of its bits"""
    t = t.detach().contiguous().cpu()
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int32).numpy().view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table(desc):
    return torch.from_numpy(desc.view(np.uint8)).to(DEV)


def i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


# ================================================================================================ 1. pk_pack_weights, direct
#             mode  N   C   T
PACK_DESCS = [(0, 5, 3, 9),        # 360 elements: one partial block
              (0, 32, 32, 1),      # 1024: exactly one full block, the next descriptor starts on a block boundary
              (0, 40, 78, 1),      # 3200: three full blocks and a partial one
              (1, 17, 12, 9),      # 2592: flipped taps over several blocks, Np 24
              (1, 8, 8, 9),        # 576: no padding at all
              (2, 13, 78, 1),      # 1248: transposed, Np 16
              (2, 24, 24, 1)]      # 576: transposed, no padding
PACK_PLACE = [3, 0, 6, 2, 5, 1, 4]                     # order of the destinations in the flat buffer: not the table's order
PACK_GAP_AFTER, PACK_GAP = 6, 304                      # a deliberate gap behind the region of descriptor 6


def test_pack_weights_hand_built_table(L):
    from infantposeestimation_gaussianbias_amd import nnops
    rng = np.random.default_rng(100)
    srcs = [ln.normal_with_specials((N, C, T), rng) for _, N, C, T in PACK_DESCS]
    srcs_d = [dev(s) for s in srcs]
    geo = [(N, C, T, mode, ln.up(C, 8), ln.up(N, 8)) for mode, N, C, T in PACK_DESCS]
    numel = [int(np.prod(ln.pack_shape(*g))) for g in geo]
    assert numel == [360, 1024, 3200, 2592, 576, 1248, 576]
    offs, off = {}, 0
    for k in PACK_PLACE:
        offs[k] = off
        off = ln.up(off + numel[k], 8) + (PACK_GAP if k == PACK_GAP_AFTER else 0)
    assert [offs[k] for k in range(len(geo))] != sorted(offs.values()) and all(o % 8 == 0 for o in offs.values())
    total = off + GUARD                                  # a tail beyond the last region
    desc = np.array([(srcs_d[k].data_ptr(), offs[k], N, C, T, mode, Cp, Np, numel[k]) for k, (N, C, T, mode, Cp, Np) in enumerate(geo)],
                    dtype=nnops._PACK_DTYPE)
    blk_desc, blk_first, nb = ln.block_table_ref(numel, 1024)
    assert nb == 1 + 1 + 4 + 3 + 1 + 2 + 1
    flat = sent16(total)
    L.call("pk_pack_weights", flat, table(desc), i32(blk_desc), i32(blk_first), nb, stream())
    torch.cuda.synchronize()
    got = bits(flat)
    outside = np.ones(total, bool)
    for k, g in enumerate(geo):
        ref = ln.pack_ref(srcs[k], *g)
        region = got[offs[k]:offs[k] + numel[k]]
        outside[offs[k]:offs[k] + numel[k]] = False
        what = f"descriptor {k} (mode {g[3]}, N {g[0]}, C {g[1]}, T {g[2]}, at {offs[k]})"
        unwritten = np.flatnonzero(region == ln.BF16_SENTINEL)
        assert unwritten.size == 0, f"{what}: {unwritten.size} elements never written, first {unwritten[0]} (block {unwritten[0] // 1024})"
        ln.assert_bits(region, ln.bf16_bits(ref).reshape(-1), what, np.isnan(ref))
        pad = ln.pack_pad_mask(*g).reshape(-1)
        assert (region[pad] == 0).all(), f"{what}: a padded lane is not +0"
    assert int(outside.sum()) >= GUARD + PACK_GAP
    touched = np.flatnonzero(outside & (got != ln.BF16_SENTINEL))
    assert touched.size == 0, f"{touched.size} elements outside every region were written, first at {touched[0]}"


# ================================================================================================ 2. WeightCache end to end
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c3 = torch.nn.Conv2d(3, 20, 3)
        self.c1 = torch.nn.Conv2d(20, 17, 1)
        self.fc = torch.nn.Linear(20, 52)
        self.shared = torch.nn.Conv2d(3, 20, 3)
        self.shared.weight = self.c3.weight              # one entry, not two


def _check_cache(wc, weights, when):
    torch.cuda.synchronize()
    for name, w in weights.items():
        src = w.detach().cpu().numpy()
        N, C = src.shape[:2]
        T = src.shape[2] * src.shape[3] if src.ndim == 4 else 1
        Cp, Np = ln.up(C, 8), ln.up(N, 8)
        f_ref = ln.pack_ref(src, N, C, T, 0, Cp, Np)
        d_ref = ln.pack_ref(src, N, C, T, 1 if T > 1 else 2, Cp, Np).reshape(C, T, Np)
        f, d = wc.fwd[id(w)], wc.dgrad[id(w)]
        assert tuple(f.shape) == (N, T, Cp) and tuple(d.shape) == (C, T, Np) and f.dtype == d.dtype == torch.bfloat16, (name, f.shape, d.shape)
        ln.assert_bits(bits(f), ln.bf16_bits(f_ref), f"{when}: fwd copy of {name}", np.isnan(f_ref))
        ln.assert_bits(bits(d), ln.bf16_bits(d_ref), f"{when}: dgrad copy of {name}", np.isnan(d_ref))


def test_weight_cache_end_to_end(L):
    from infantposeestimation_gaussianbias_amd import nnops
    rng = np.random.default_rng(200)
    net = _Net().to(DEV)
    weights = {"c3": net.c3.weight, "c1": net.c1.weight, "fc": net.fc.weight}
    with torch.no_grad():
        for w in weights.values():
            w.copy_(dev(ln.normal_with_specials(tuple(w.shape), rng)))
    wc = nnops.WeightCache(net)
    assert len(wc.entries) == 3 and net.shared.weight is net.c3.weight
    wc.ensure_fresh()
    assert set(wc.fwd) == set(wc.dgrad) == {id(w) for w in weights.values()}
    _check_cache(wc, weights, "first pack")
    # the regions tile the flat buffer: 8-aligned, disjoint, nothing but the rounding gaps between them
    base = wc.flat.data_ptr()
    spans = sorted(((v.data_ptr() - base) // 2, v.numel()) for v in list(wc.fwd.values()) + list(wc.dgrad.values()))
    assert spans[0][0] == 0 and all(o % 8 == 0 for o, _ in spans)
    assert all(o1 == ln.up(o0 + n0, 8) for (o0, n0), (o1, _) in zip(spans, spans[1:])) and wc.flat.numel() == ln.up(sum(spans[-1]), 8)

    # nothing changed: nothing is launched (the sentinel written over the whole buffer is still there)
    wc.flat.view(torch.int16).fill_(ln.BF16_SENTINEL)
    wc.ensure_fresh()
    torch.cuda.synchronize()
    assert (bits(wc.flat) == ln.BF16_SENTINEL).all(), "ensure_fresh() launched although no weight had changed"

    # an in-place torch write is seen through the version counter
    with torch.no_grad():
        net.c1.weight.mul_(2)
    wc.ensure_fresh()
    _check_cache(wc, weights, "after mul_(2)")

    # a write behind torch's back (through .data, as the fused optimiser writes through raw pointers) needs mark_dirty()
    wc.flat.view(torch.int16).fill_(ln.BF16_SENTINEL)
    net.fc.weight.data.copy_(dev(ln.normal_with_specials((52, 20), rng)))
    net.c3.weight.data.mul_(-0.5)
    wc.mark_dirty()
    wc.ensure_fresh()
    _check_cache(wc, weights, "after mark_dirty()")
    wc.flat.view(torch.int16).fill_(ln.BF16_SENTINEL)
    wc.ensure_fresh()
    torch.cuda.synchronize()
    assert (bits(wc.flat) == ln.BF16_SENTINEL).all(), "ensure_fresh() launched again after the refresh"


# ================================================================================================ 3. pk_embed_boxes, direct
#             real box r[4]         twin box p[4]
EMBED_BOXES = [([1, 1, 1, 78], [1, 1, 1, 80]),               # plain 1-D
               ([1, 1, 156, 78], [1, 1, 160, 80]),           # plain 2-D: 12168 elements, 12 blocks, the last one partial
               ([18, 18, 3, 3], [24, 24, 3, 3]),             # conv
               ([3, 2, 39, 78], [3, 2, 40, 80]),             # qkv weight, 2 heads of 39
               ([1, 3, 2, 39], [1, 3, 2, 40]),               # qkv bias
               ([1, 78, 2, 39], [1, 80, 2, 40]),             # proj weight
               ([1, 1, 32, 64], [1, 1, 32, 64]),             # unpadded, exactly 2048 elements
               ([1, 1, 1, 1], [1, 1, 1, 1])]                 # one element
EMBED_PLACE = [1, 7, 3, 0, 6, 2, 5, 4]                       # order inside the twin: not the table's order
REAL_GAP = 16


class _Boxes:
    """The table of EMBED_BOXES over one flat twin (4-aligned offsets, a sentinel tail) and one flat buffer of real tensors (sentinel gaps)."""

    def __init__(self):
        from infantposeestimation_gaussianbias_amd.models import padded
        self.numel = [int(np.prod(r)) for r, _ in EMBED_BOXES]
        self.toff, off = {}, 0
        for k in EMBED_PLACE:
            self.toff[k] = off
            off = ln.up(off + int(np.prod(EMBED_BOXES[k][1])), 4)
        self.twin_used, self.twin_total = off, off + GUARD
        self.roff, off = [], REAL_GAP
        for n in self.numel:
            self.roff.append(off)
            off = ln.up(off + n, 4) + REAL_GAP
        self.real_total = off
        self.real = sent32(self.real_total)
        self.twin = sent32(self.twin_total)
        rows = [(self.real.data_ptr() + 4 * self.roff[k], self.toff[k], r, p) for k, (r, p) in enumerate(EMBED_BOXES)]
        self.table = padded._Table(rows, DEV)
        assert self.table.nb == sum(-(-n // 1024) for n in self.numel) and self.numel[1] == 12168 and self.numel[6] == 2048
        self.in_box = ln.box_mask(self.twin_total, [(self.toff[k], r, p) for k, (r, p) in enumerate(EMBED_BOXES)])
        self.in_real = np.zeros(self.real_total, bool)
        for o, n in zip(self.roff, self.numel):
            self.in_real[o:o + n] = True

    def set_real(self, arrays):
        host = np.full(self.real_total, ln.F32_SENTINEL, np.uint32)
        for o, a in zip(self.roff, arrays):
            host[o:o + a.size] = a.reshape(-1).view(np.uint32)
        self.real.copy_(dev(host.view(np.float32)))

    def reals(self, host_bits):
        return [host_bits[o:o + n] for o, n in zip(self.roff, self.numel)]

    def boxes(self, twin_host):
        return [ln.box_view(twin_host, self.toff[k], r, p).reshape(-1) for k, (r, p) in enumerate(EMBED_BOXES)]

    def run(self, direction):
        self.table.run(self.twin, direction)
        torch.cuda.synchronize()


def _name(k):
    return f"box {k} (real {EMBED_BOXES[k][0]} in twin {EMBED_BOXES[k][1]})"


def test_embed_boxes_real_to_twin(L):
    rng = np.random.default_rng(300)
    bx = _Boxes()
    src = [ln.normal_with_specials(tuple(r), rng) for r, _ in EMBED_BOXES]
    bx.set_real(src)
    real_before = bits(bx.real)
    bx.run(0)
    got = bits(bx.twin)
    for k, (box, s) in enumerate(zip(bx.boxes(got), src)):
        ln.assert_bits(box, s.reshape(-1).view(np.uint32), _name(k), np.isnan(s))
    touched = np.flatnonzero(~bx.in_box & (got != ln.F32_SENTINEL))
    assert touched.size == 0, f"{touched.size} twin elements outside every box were written, first at {touched[0]}"
    assert int((~bx.in_box).sum()) > GUARD + 80 * 160 - 78 * 156
    assert np.array_equal(bits(bx.real), real_before), "direction 0 wrote to a real tensor"


def test_embed_boxes_twin_to_real(L):
    rng = np.random.default_rng(301)
    bx = _Boxes()
    twin = ln.normal_with_specials((bx.twin_total,), rng)
    bx.twin.copy_(dev(twin))
    bx.run(1)
    got = bits(bx.real)
    want = bx.boxes(twin)
    for k, (g, w) in enumerate(zip(bx.reals(got), want)):
        ln.assert_bits(g, np.ascontiguousarray(w).view(np.uint32), _name(k), np.isnan(w))
    assert (got[~bx.in_real] == ln.F32_SENTINEL).all(), "direction 1 wrote between the real tensors"
    assert np.array_equal(bits(bx.twin), twin.view(np.uint32)), "direction 1 wrote to the twin"


def test_embed_boxes_accumulate(L):
    rng = np.random.default_rng(302)
    bx = _Boxes()
    twin = rng.standard_normal(bx.twin_total).astype(np.float32)
    real0 = [rng.standard_normal(tuple(r)).astype(np.float32) for r, _ in EMBED_BOXES]
    bx.twin.copy_(dev(twin))
    bx.set_real(real0)
    want = [a.reshape(-1) for a in real0]
    for launch in (1, 2):
        bx.run(2)
        got = bits(bx.real)
        want = [w + np.ascontiguousarray(b) for w, b in zip(want, bx.boxes(twin))]          # one fp32 add per launch
        assert all(w.dtype == np.float32 for w in want)
        for k, (g, w) in enumerate(zip(bx.reals(got), want)):
            ln.assert_bits(g, w.view(np.uint32), f"launch {launch}, {_name(k)}")
        assert (got[~bx.in_real] == ln.F32_SENTINEL).all(), "direction 2 wrote between the real tensors"
    assert np.array_equal(bits(bx.twin), twin.view(np.uint32)), "direction 2 wrote to the twin"


# ================================================================================================ 4. PaddedTwin on the two twin models
MODELS = {"hrformer_base": ("hrformer_base", 13, "fusion", "hrformer_base_fusion_k13", 44),
          "hrnet_w18": ("hrnet_w18", 17, "heatmap", "hrnet_w18_heatmap", 41)}


@pytest.fixture(scope="module", params=sorted(MODELS))
def twin_model(request, golden):
    """(real model on the device in training mode, its PaddedTwin); built once per model.  Every test leaves the real parameters and
    buffers, the twin's flat storage and the twin's gradient buffer as it found them."""
    from infantposeestimation_gaussianbias_amd.models import PoseEstimator
    from infantposeestimation_gaussianbias_amd.models.padded import twin_for
    backbone, K, head, spec, salt = MODELS[request.param]
    m = PoseEstimator(backbone, K, False, head, True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(golden("state_keys.json")[spec], salt).items()}, strict=True)
    m = m.to(DEV).train()
    tw = twin_for(m)
    assert tw is not None, f"{backbone} runs as a padded twin"
    return m, tw


def _heads_of(real, name):
    """head count of the attention block a parameter belongs to (from the real model's modules), None for everything else"""
    if ".attn." not in name:
        return None
    block = dict(real.named_modules())[name.rsplit(".attn.", 1)[0]]
    assert block.dim % block.heads == 0
    return block.heads


def _twin_tensors(tw):
    """[(key, real tensor, twin tensor)]: parameters, then float buffers ("#" + name), paired by name"""
    rp, tp = dict(tw.real.named_parameters()), dict(tw.twin.named_parameters())
    rb = {k: v for k, v in tw.real.named_buffers() if v.is_floating_point()}
    tb = {k: v for k, v in tw.twin.named_buffers() if v.is_floating_point()}
    assert list(rp) == list(tp) and list(rb) == list(tb)
    return [(k, rp[k], tp[k]) for k in tp] + [("#" + k, rb[k], tb[k]) for k in tb]


def _masks(tw):
    """{key: mask over the twin tensor of the elements that belong to the real tensor}, derived from names and head counts"""
    out = {}
    for k, r, t in _twin_tensors(tw):
        out[k] = ln.embed_by_name(k, np.zeros(tuple(r.shape), np.float32), tuple(t.shape), _heads_of(tw.real, k.lstrip("#")))[1]
    return out


def _flat_offset(tw, t):
    off = (t.data_ptr() - tw.flat.data_ptr()) // 4
    assert 0 <= off and off + t.numel() <= tw.flat.numel(), "a twin tensor does not live in the twin's flat storage"
    return off


def test_twin_sync_embeds_every_tensor(twin_model):
    m, tw = twin_model
    tw.mark_dirty()
    tw.sync_to_twin()
    torch.cuda.synchronize()
    flat = bits(tw.flat)
    covered = np.zeros(flat.size, bool)
    n_padded = n_struct = 0
    for k, r, t in _twin_tensors(tw):
        heads = _heads_of(m, k.lstrip("#"))
        want, mask = ln.embed_by_name(k, r.detach().cpu().numpy(), tuple(t.shape), heads)
        off = _flat_offset(tw, t)
        assert not covered[off:off + t.numel()].any(), f"{k} overlaps another twin tensor"
        covered[off:off + t.numel()] = True
        ln.assert_bits(flat[off:off + t.numel()], want.reshape(-1).view(np.uint32), f"{k} {tuple(r.shape)} in {tuple(t.shape)}")
        ln.assert_bits(bits(t).reshape(-1), want.reshape(-1).view(np.uint32), f"{k} read through the twin's parameter")
        assert (want.reshape(-1).view(np.uint32)[~mask.reshape(-1)] == 0).all()
        n_padded += tuple(r.shape) != tuple(t.shape)
        n_struct += heads is not None and tuple(r.shape) != tuple(t.shape) and k.endswith(("qkv.weight", "qkv.bias", "proj.weight"))
    assert (flat[~covered] == 0).all(), "the alignment gaps of the twin's flat storage are not +0"
    assert n_padded > 50, "hardly any tensor of the twin is padded"
    if m.head_type == "fusion":                          # HRFormer-base: 39 -> 40 per head in every block of stages 2 to 4
        assert n_struct >= 3, "no head-structured tensor was checked"


def test_twin_grads_to_real_accumulates(twin_model):
    m, tw = twin_model
    tw.sync_to_twin()
    masks = _masks(tw)
    saved = tw.grad.clone()
    tp = dict(tw.twin.named_parameters())
    g = torch.Generator(device=DEV).manual_seed(7)
    try:
        tw.grad.copy_(torch.randn(tw.grad.shape, generator=g, device=DEV))
        for p in m.parameters():
            p.grad = None
        used_before = {k: t._pk_used for k, t in tp.items()}
        for launch in (1, 2):
            for t in tp.values():
                t._pk_used = True
            tw._pending = True
            tw.grads_to_real()
            torch.cuda.synchronize()
            assert tw._pending is False
            for k, p in m.named_parameters():
                sink = tp[k]._pk_grad_sink
                assert sink.data_ptr() == tw.grad.data_ptr() + 4 * _flat_offset(tw, tp[k]) and sink.shape == tp[k].shape
                box = sink.detach().cpu().numpy()[masks[k]]
                want = box if launch == 1 else box + box
                assert p.grad is not None and p.grad.shape == p.shape, k
                ln.assert_bits(bits(p.grad).reshape(-1), np.ascontiguousarray(want).view(np.uint32), f"launch {launch}: .grad of {k}")
        for k, t in tp.items():
            t._pk_used = used_before[k]
    finally:
        tw.grad.copy_(saved)
        for p in m.parameters():
            p.grad = None


def test_twin_buffers_to_real(twin_model):
    m, tw = twin_model
    tw.sync_to_twin()
    masks = _masks(tw)
    flat_saved = tw.flat.clone()
    pairs = [(k, r, t) for k, r, t in _twin_tensors(tw) if k.startswith("#")]
    assert pairs and any(k.endswith("running_var") for k, _, _ in pairs)
    real_saved = [r.detach().clone() for _, r, _ in pairs]
    g = torch.Generator(device=DEV).manual_seed(8)
    try:
        with torch.no_grad():
            for _, _, t in pairs:
                t.copy_(torch.randn(t.shape, generator=g, device=DEV))           # the padding too: it must not travel
        tw.buffers_to_real()
        torch.cuda.synchronize()
        for k, r, t in pairs:
            want = t.detach().cpu().numpy()[masks[k]]
            ln.assert_bits(bits(r).reshape(-1), np.ascontiguousarray(want).view(np.uint32), f"real buffer {k[1:]}")
    finally:
        with torch.no_grad():
            tw.flat.copy_(flat_saved)
            for (_, r, _), s in zip(pairs, real_saved):
                r.copy_(s)
        tw.mark_dirty()


def test_twin_padding_stays_zero_through_a_training_step(twin_model):
    """padded.py's claim: zero weights and biases keep every padded channel exactly zero.  After one train-mode forward and backward
    every element of the twin's flat storage outside the boxes -- parameters and running statistics alike -- is still +0 or -0."""
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    m, tw = twin_model
    K = m.num_keypoints
    batch = synthetic_batch(1, (64, 64), (16, 16), K, 2.0, DEV, seed=3)
    x = dev(synth_input("layout_twin_step", (1, 3, 64, 64)))
    for p in m.parameters():
        p.grad = None
    try:
        if m.head_type == "fusion":
            o = m(x, batch["target"], batch["target_weight"], batch["keypoints"], input_size=(64, 64))
        else:
            o = m(x, batch["target"], batch["target_weight"])
        o["loss"].backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(o["loss"].detach()))
        assert sum(p.grad is not None for p in m.parameters()) > 100, "the backward pass did not reach the real parameters"
        flat = bits(tw.flat)
        covered = np.zeros(flat.size, bool)
        dirty = []
        for k, r, t in _twin_tensors(tw):
            mask = ln.embed_by_name(k, np.zeros(tuple(r.shape), np.float32), tuple(t.shape), _heads_of(m, k.lstrip("#")))[1].reshape(-1)
            off = _flat_offset(tw, t)
            covered[off:off + t.numel()] = True
            body = flat[off:off + t.numel()]
            bad = ~mask & ((body & 0x7FFFFFFF) != 0)
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                dirty.append(f"{k} {tuple(t.shape)}: {int(bad.sum())} padded elements, first at {np.unravel_index(i, tuple(t.shape))} = "
                             f"{body[i:i + 1].view(np.float32)[0]!r}")
        assert not dirty, "padding of the twin is no longer zero in " + "; ".join(dirty[:20]) + f" ({len(dirty)} tensors)"
        assert ((flat[~covered] & 0x7FFFFFFF) == 0).all(), "the alignment gaps of the twin's flat storage are no longer zero"
    finally:
        for p in m.parameters():
            p.grad = None


def test_twin_grads_to_real_overwrites_gradient_sinks(twin_model):
    """With engine.FlatAdamW attached the real parameters carry gradient sinks: the extraction stores into them, it does not add."""
    from infantposeestimation_gaussianbias_amd import engine, nnops
    m, tw = twin_model
    tw.sync_to_twin()
    masks = _masks(tw)
    saved = tw.grad.clone()
    tp = dict(tw.twin.named_parameters())
    for p in m.parameters():
        p.grad = None
    opt = engine.FlatAdamW(m, direct_grads=True)
    opt.install_grad_views()
    g = torch.Generator(device=DEV).manual_seed(9)
    try:
        assert all(getattr(p, "_pk_grad_sink", None) is not None for p in m.parameters())
        tw.grad.copy_(torch.randn(tw.grad.shape, generator=g, device=DEV))
        opt.grad.view(torch.int32).fill_(ln.F32_SENTINEL)
        for launch in (1, 2):
            nnops.begin_grad_epoch()
            for t in tp.values():
                t._pk_used = True
            tw._pending = True
            tw.grads_to_real()
            torch.cuda.synchronize()
            for i, (k, p) in enumerate(zip(opt.names, opt.params)):
                want = tp[k]._pk_grad_sink.detach().cpu().numpy()[masks[k]]
                ln.assert_bits(bits(opt.grad_view(i)).reshape(-1), np.ascontiguousarray(want).view(np.uint32), f"launch {launch}: sink of {k}")
        for t in tp.values():
            t._pk_used = False
    finally:
        tw.grad.copy_(saved)
        for p in m.parameters():
            p.grad = None
            if hasattr(p, "_pk_grad_sink"):
                del p._pk_grad_sink
        tw.mark_dirty()


# ================================================================================================ 5. pk_nchw_f32_to_nhwc_bf16
def _to_nhwc(L, x, sp, Cpad):
    B, Cin, H, W = x.shape
    n = B * H * W * Cpad
    buf = sent16(n + GUARD)
    xd = dev(x)
    spd = None if sp is None else dev(sp)
    L.call("pk_nchw_f32_to_nhwc_bf16", xd, spd, buf, B, Cin, H, W, Cpad, stream())
    torch.cuda.synchronize()
    got = bits(buf)
    assert (got[n:] == ln.BF16_SENTINEL).all(), "wrote past the end of the output"
    return got[:n].reshape(B, H, W, Cpad)


@pytest.mark.parametrize("Cin,Cpad,shape", [(3, 8, (2, 9, 7)), (8, 8, (2, 9, 7)), (13, 16, (2, 9, 7)), (17, 24, (2, 9, 7)),
                                            (3, 8, (3, 600, 583))])           # 1 049 400 pixels: past 4096 x 256, no multiple of 256
def test_nchw_to_nhwc_plain(L, Cin, Cpad, shape):
    B, H, W = shape
    rng = np.random.default_rng(500 + Cin + H)
    x = ln.normal_with_specials((B, Cin, H, W), rng)
    got = _to_nhwc(L, x, None, Cpad)
    ref = ln.nhwc_ref(x, Cpad)
    unwritten = np.flatnonzero(got.reshape(-1) == ln.BF16_SENTINEL)
    assert unwritten.size == 0, f"{unwritten.size} elements never written, first {unwritten[0]} (pixel {unwritten[0] // Cpad})"
    ln.assert_bits(got, ln.bf16_bits(ref), f"Cin {Cin}, Cpad {Cpad}, {shape}", np.isnan(ref))
    assert (got[..., Cin:] == 0).all(), "a padded channel is not +0"


@pytest.mark.parametrize("Cin,Cpad", [(17, 24), (13, 16)])
def test_nchw_to_nhwc_softplus_derivative(L, Cin, Cpad):
    B, H, W = 2, 64, 48
    rng = np.random.default_rng(510 + Cin)
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    z = np.maximum(1.5 * rng.standard_normal((B, Cin, H, W)), -3.0)
    sp = np.log1p(np.exp(z)).astype(np.float32)                      # softplus(z), the head's fp32 output
    assert (1.0 - np.exp(-sp.astype(np.float64))).min() >= 0.047
    got = _to_nhwc(L, x, sp, Cpad)
    assert (got[..., Cin:] == 0).all(), "a padded channel is not +0"
    got = got[..., :Cin].transpose(0, 3, 1, 2)
    rne, lo, hi, inside = ln.softplus_window(x, sp)
    mismatch = got != rne
    share = float(inside.mean())
    print(f"softplus path Cin {Cin}: {100 * share:.4f} % of {got.size} elements within the window of a rounding boundary, "
          f"{int(mismatch.sum())} differ from RNE(r), {int((mismatch & ~inside).sum())} of them outside the window")
    assert share <= 0.005, share
    far = mismatch & ~inside
    if far.any():
        i = np.unravel_index(int(np.flatnonzero(far)[0]), far.shape)
        raise AssertionError(f"{int(far.sum())} elements away from every rounding boundary differ from RNE(r), first at {i}: got "
                             f"{int(got[i]):#x}, reference {int(rne[i]):#x} (x {x[i]!r}, softplus {sp[i]!r})")
    assert ((got == lo) | (got == hi))[inside].all(), "an element near a rounding boundary is neither of its two neighbours"


# ================================================================================================ 6. row moves and DropPath, grid wrapped
ROW_CASES = [(33000, 128), (3001, 4), (3001, 12)]           # 33 000 x 32 dwords = 1 056 000 > 4096 x 256


@pytest.mark.parametrize("n_rows,row_bytes", ROW_CASES)
def test_rows_by_map_gather(L, n_rows, row_bytes):
    dw = row_bytes // 4
    rng = np.random.default_rng(600 + row_bytes)
    n_src = n_rows - n_rows // 11
    src = rng.integers(1, 2 ** 32, (n_src, dw), dtype=np.uint64).astype(np.uint32)
    rowmap = rng.integers(0, n_src, n_rows).astype(np.int32)
    rowmap[rng.random(n_rows) < 0.1] = -1
    rowmap[[0, n_rows - 1]] = [n_src - 1, -1]
    assert 0.05 < (rowmap < 0).mean() < 0.15
    buf = sent32(n_rows * dw + GUARD)
    L.call("pk_rows_by_map", dev(src.view(np.float32)), buf, dev(rowmap), n_rows, row_bytes, 0, stream())
    torch.cuda.synchronize()
    got = bits(buf)
    assert (got[n_rows * dw:] == ln.F32_SENTINEL).all(), "wrote past the end of the destination"
    ln.assert_bits(got[:n_rows * dw], ln.rows_gather_ref(src, rowmap).reshape(-1), f"gather of {n_rows} rows of {row_bytes} bytes")
    assert not got[:n_rows * dw].reshape(n_rows, dw)[rowmap < 0].any(), "a row mapped to -1 is not all-zero bits"


@pytest.mark.parametrize("n_rows,row_bytes", ROW_CASES)
def test_rows_by_map_scatter(L, n_rows, row_bytes):
    dw = row_bytes // 4
    rng = np.random.default_rng(610 + row_bytes)
    n_dst = n_rows + n_rows // 9
    src = rng.integers(1, 2 ** 32, (n_rows, dw), dtype=np.uint64).astype(np.uint32)
    src[src == ln.F32_SENTINEL] = 1
    rowmap = rng.permutation(n_dst)[:n_rows].astype(np.int32)           # injective
    rowmap[rng.random(n_rows) < 0.1] = -1
    rowmap[[0, n_rows - 1]] = [-1, -1]
    assert 0.05 < (rowmap < 0).mean() < 0.15
    front = max(GUARD, dw)                                               # room in front: row -1 of a missing guard would land here
    buf = sent32(front + n_dst * dw + GUARD)
    dst = buf[front:front + n_dst * dw]
    L.call("pk_rows_by_map", dev(src.view(np.float32)), dst, dev(rowmap), n_rows, row_bytes, 1, stream())
    torch.cuda.synchronize()
    got = bits(buf)
    assert (got[:front] == ln.F32_SENTINEL).all(), "wrote in front of the destination (a row mapped to -1 was stored)"
    assert (got[front + n_dst * dw:] == ln.F32_SENTINEL).all(), "wrote past the end of the destination"
    want = ln.rows_scatter_ref(src, rowmap, np.full((n_dst, dw), ln.F32_SENTINEL, np.uint32))
    ln.assert_bits(got[front:front + n_dst * dw], want.reshape(-1), f"scatter of {n_rows} rows of {row_bytes} bytes")
    hit = np.zeros(n_dst, bool)
    hit[rowmap[rowmap >= 0]] = True
    assert (got[front:front + n_dst * dw].reshape(n_dst, dw)[~hit] == ln.F32_SENTINEL).all(), "a row no entry maps to was written"


@pytest.mark.parametrize("keep", [0.9, 0.75])
def test_drop_path_grid_wrapped(L, keep):
    batch, per = 67, 15731                                               # 1 053 977 elements: past 4096 x 256, no multiple of 256
    rng = np.random.default_rng(620)
    x = rng.standard_normal((batch, per)).astype(np.float32)
    xb = x.reshape(-1).view(np.uint32)
    xb[[0, 5, 77, per, batch * per - 1]] = [0x80000000, 0x00000000, 0x00000001, 0x7F7FFFFF, 0x807FFFFF]
    mask = (rng.random(batch) < keep).astype(np.float32)
    mask[[0, 1, batch - 1]] = [1.0, 0.0, 1.0]
    buf = sent32(batch * per + GUARD)
    L.call("pk_drop_path_f32", dev(x), dev(mask), buf, batch, per, float(keep), stream())
    torch.cuda.synchronize()
    got = bits(buf)
    assert (got[batch * per:] == ln.F32_SENTINEL).all(), "wrote past the end of the output"
    with np.errstate(over="ignore", invalid="ignore"):
        ref = ln.drop_path_ref(x, mask, keep)
    assert ref.dtype == np.float32
    ln.assert_bits(got[:batch * per], ref.reshape(-1).view(np.uint32), f"drop_path keep {keep}", np.isnan(ref))
