"""GPU tests of the per-tensor statistics (csrc/pk_tensor_stats.hip: pk_tensor_stats, pk_tensor_stats_latch) against the numpy
restatement tests/tensor_stats_np.py, and of their use by engine.FlatAdamW / engine.Trainer.

C = pk_tensor_stats_chunk_elems(), the elements of one plan item; every shape below is derived from it.  Counts, min and max are
compared exactly.  The three sums are fp64 sums of exactly representable terms in another order than the restatement's: each lies within
n 2^-52 (its own absolute sum) of the exact value (tensor_stats_np.sum_bound), derived, not measured.  Only NaN / inf VALUES go through
ordinary arithmetic here; every index stays inside its buffer."""
import math

import numpy as np
import pytest
import torch

import tensor_stats_np as tnp

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def ops():
    from infantposeestimation_gaussianbias_amd import hipops
    return hipops


@pytest.fixture(scope="module")
def C(ops):
    return ops.tensor_stats_chunk_elems()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _records(ops, flat, offsets, counts, b=None, flags=None, tiny=0.0):
    plan = ops.TensorStatsPlan(offsets, counts, DEV)
    rec = ops.tensor_stats(plan, _up(flat), None if b is None else _up(b), None if flags is None else _up(flags), tiny)
    return ops.tensor_stats_records(rec).copy()


def _check(rec, want, what=""):
    """One device record against the restatement's: counts, min, max exact; sums within the summation bound."""
    for k in ("n", "nonfinite", "small", "zero"):
        assert int(rec[k]) == want[k], (what, k, int(rec[k]), want[k])
    for k in ("min", "max"):
        assert rec[k] == want[k], (what, k, rec[k], want[k])
    m = want["n"] - want["nonfinite"]
    for k, scale in (("sum", want["sumabs"]), ("sumsq", want["sumsq"]), ("sumabs", want["sumabs"])):
        assert abs(float(rec[k]) - want[k]) <= tnp.sum_bound(m, scale), (what, k, float(rec[k]), want[k], tnp.sum_bound(m, scale))


def _check_all(ops, tensors, flags_of=None, tiny=0.0, **kw):
    flat, offsets, counts = tnp.pack(tensors)
    flags = None
    if flags_of is not None:
        flags = np.zeros(flat.size, np.uint8)
        for o, f in zip(offsets, flags_of):
            flags[o:o + f.size] = f
    recs = _records(ops, flat, offsets, counts, flags=flags, tiny=tiny, **kw)
    assert len(recs) == len(tensors)
    for i, t in enumerate(tensors):
        _check(recs[i], tnp.record_np(t, None if flags_of is None else flags_of[i], tiny), f"tensor {i} ({t.size} elements)")
    return recs


# ------------------------------------------------------------------------------------------------ 1. tails and chunk edges
def test_tails_and_chunk_edges(ops, C):
    """Every count around a float4, a wave's single pass (256) and an item (C), with poisoned padding behind each tensor, scales from
    1e-20 to 1e20 and one tensor of +-FLT_MAX (its squares and their sum need fp64)."""
    counts = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 5 * C + 3]
    rng = np.random.default_rng(1)
    scales = 10.0 ** np.linspace(-20, 20, len(counts))
    tensors = [(s * rng.standard_normal(c)).astype(np.float32) for c, s in zip(counts, scales)]
    big = counts.index(C + 1)
    tensors[big] = np.where(rng.random(C + 1) < 0.5, FLT_MAX, -FLT_MAX).astype(np.float32)
    flat, offsets, _ = tnp.pack(tensors)
    pad = np.ones(flat.size, bool)
    for o, c in zip(offsets, counts):
        pad[o:o + c] = False
    assert pad.sum() >= 10 and np.isnan(flat[pad][0::2]).all() and (flat[pad][1::2] == np.float32(1e38)).all()
    recs = _check_all(ops, tensors)
    assert (recs["nonfinite"] == 0).all() and np.array_equal(recs["n"], counts)
    assert recs["sumsq"][big] == pytest.approx((C + 1) * float(FLT_MAX) ** 2, rel=1e-12) and math.isfinite(recs["sumsq"][big])
    assert recs["min"][big] == -FLT_MAX and recs["max"][big] == FLT_MAX


# ------------------------------------------------------------------------------------------------ 2. long and short
def test_one_long_tensor_and_its_small_neighbour(ops, C):
    """300 C + 1 elements: 301 partials, more than the finalize wave's 64 lanes (and than a 256-lane workgroup) take in one pass; the
    3-element neighbour behind it catches an off-by-one in the partial ranges."""
    rng = np.random.default_rng(2)
    tensors = [rng.standard_normal(300 * C + 1).astype(np.float32), np.array([5.0, -7.0, 0.25], np.float32),
               rng.standard_normal(65 * C).astype(np.float32)]
    recs = _check_all(ops, tensors)
    assert (recs["sum"][1], recs["sumsq"][1], recs["min"][1], recs["max"][1], recs["n"][1]) == (-1.75, 74.0625, -7.0, 5.0, 3)


def test_three_thousand_short_tensors(ops, C):
    rng = np.random.default_rng(3)
    tensors = [rng.standard_normal(1 + i % 64).astype(np.float32) * np.float32(1 + i % 7) for i in range(3000)]
    flat, offsets, counts = tnp.pack(tensors)
    assert ops.tensor_stats_plan_host(offsets, counts)[1] == 3000          # one item, i.e. one wave, each
    _check_all(ops, tensors)


# ------------------------------------------------------------------------------------------------ 3. non-finite placement
def test_nonfinite_placement(ops, C):
    """NaN, +inf, -inf at a tensor's first and last element and on both sides of an item edge: counted, and the rest of the record is
    that of the same data without them."""
    rng = np.random.default_rng(4)
    specials = [np.nan, np.inf, -np.inf]
    tensors, cleaned = [], []
    for k, bad in enumerate(specials):
        for n in (1, 6, 257, 3 * C + 2):
            t = rng.standard_normal(n).astype(np.float32)
            where = sorted({0, n - 1} | ({C - 1, C} if n > C else set()))
            t[where] = bad
            tensors.append(t)
            cleaned.append(np.delete(t, where))
    tensors.append(np.full(C + 5, np.nan, np.float32))          # NaN throughout
    cleaned.append(np.zeros(0, np.float32))
    recs = _check_all(ops, tensors)
    for i, (t, c) in enumerate(zip(tensors, cleaned)):
        want = tnp.record_np(c) if c.size else None
        assert recs["n"][i] == t.size and recs["nonfinite"][i] == t.size - c.size > 0
        if want is None:
            assert (recs["sum"][i], recs["sumsq"][i], recs["sumabs"][i]) == (0.0, 0.0, 0.0)
            assert recs["min"][i] == np.inf and recs["max"][i] == -np.inf and recs["small"][i] == 0
        else:
            assert recs["min"][i] == want["min"] and recs["max"][i] == want["max"]
            m = c.size
            for k, scale in (("sum", want["sumabs"]), ("sumsq", want["sumsq"]), ("sumabs", want["sumabs"])):
                assert abs(recs[k][i] - want[k]) <= tnp.sum_bound(m, scale), (i, k)


# ------------------------------------------------------------------------------------------------ 4. flags
def _mixed_flags(n, seed):
    """test_gpu_grad_guard.py's _mixed: flags alternate active (2 / 3) and inactive (0 / 1) runs of 1..37 elements, starting active."""
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 38, size=n // 10 + 2)
    edges = np.minimum(np.cumsum(runs), n)
    run_of = np.searchsorted(edges, np.arange(n), side="right")
    inactive = (run_of & 1) == 1
    flags = np.where(inactive, run_of % 4 // 2, 2 + (run_of // 2) % 2).astype(np.uint8)
    return flags, inactive


def test_flags(ops, C):
    """Whole tensors inactive (flags 0 / 1) and full of NaN and 1e38: n = 0 and an empty record.  Inside a tensor, alternating runs whose
    inactive elements hold the same poison: only the active ones count."""
    rng = np.random.default_rng(5)
    tensors, flags_of = [], []
    for i, n in enumerate((3, 255, C + 1, 2 * C + 7, 5, 1000)):
        t = rng.standard_normal(n).astype(np.float32)
        if i % 2 == 0:                                              # inactive as a whole
            f = np.full(n, i % 4 // 2, np.uint8)
            t[:] = np.where(np.arange(n) % 2 == 0, np.float32(np.nan), np.float32(1e38))
        else:
            f, inactive = _mixed_flags(n, 50 + i)
            t[inactive] = np.where(np.arange(n)[inactive] % 2 == 0, np.float32(np.nan), np.float32(1e38))
        tensors.append(t)
        flags_of.append(f)
    recs = _check_all(ops, tensors, flags_of)
    assert (recs["nonfinite"] == 0).all()
    for i in (0, 2, 4):
        assert recs["n"][i] == 0 and recs["min"][i] == np.inf and recs["max"][i] == -np.inf and recs["sumsq"][i] == 0.0
    for i in (1, 3, 5):
        assert 0 < recs["n"][i] == int(((flags_of[i] & 2) != 0).sum()) < tensors[i].size


# ------------------------------------------------------------------------------------------------ 5. tiny
@pytest.mark.parametrize("tiny", [0.0, 1e-3, float(np.float32(1e-40)), 2.5])
def test_tiny(ops, C, tiny):
    t32 = np.float32(tiny)
    edge = np.array([t32, -t32, np.nextafter(t32, np.float32(np.inf)), -np.nextafter(t32, np.float32(np.inf)), -0.0, 0.0, 1e-42, -1e-42,
                     np.nextafter(t32, np.float32(0)), 1.0, np.nan, np.inf], np.float32)
    rng = np.random.default_rng(6)
    body = (rng.standard_normal(C + 9) * 2 * max(tiny, 1e-3)).astype(np.float32)
    tensors = [edge, np.concatenate([body, edge]), np.concatenate([edge, body])]
    recs = _check_all(ops, tensors, tiny=tiny)
    fin = edge[np.isfinite(edge)].astype(np.float64)
    assert recs["small"][0] == int((np.abs(fin) <= float(t32)).sum()) >= 5 and recs["n"][0] == edge.size and recs["nonfinite"][0] == 2
    assert recs["small"][0] < fin.size                                       # 1.0 and the value just above tiny are not small
    if tiny == 0.0:
        assert recs["small"][0] == int((fin == 0).sum())                     # +-0 only: not the denormals


# ------------------------------------------------------------------------------------------------ 6. difference mode
def test_difference_mode_is_the_plain_call_on_the_fp32_difference(ops, C):
    rng = np.random.default_rng(7)
    counts = [1, 3, 6, 257, C + 3, 2 * C, 3 * C + 1]
    a_t = [rng.standard_normal(c).astype(np.float32) for c in counts]
    b_t = [(t + np.float32(1e-3) * rng.standard_normal(t.size).astype(np.float32)).astype(np.float32) for t in a_t]
    a_t[4][[0, C - 1, C, C + 2]] = [np.inf, -np.inf, np.inf, np.nan]
    b_t[4][[0, C - 1, C, C + 2]] = [np.inf, -np.inf, 1.0, 2.0]          # inf - inf = NaN twice, then inf, NaN
    b_t[5][:] = a_t[5]                                                   # all zeros
    a, offsets, _ = tnp.pack(a_t)
    b, _, _ = tnp.pack(b_t)
    with np.errstate(invalid="ignore"):
        d_t = [x - y for x, y in zip(a_t, b_t)]                          # float32 - float32: one rounding
        d = a - b
    assert all(t.dtype == np.float32 for t in d_t) and np.isnan(d_t[4][0]) and np.isnan(d_t[4][C - 1])
    flags, _ = _mixed_flags(a.size, 70)
    for fl in (None, flags):
        got = _records(ops, a, offsets, counts, b=b, flags=fl, tiny=1e-4)
        plain = _records(ops, d, offsets, counts, flags=fl, tiny=1e-4)
        assert got.tobytes() == plain.tobytes()
    plain = _records(ops, a, offsets, counts, b=b)
    for i, t in enumerate(d_t):
        _check(plain[i], tnp.record_np(t), f"difference {i}")
    assert plain["nonfinite"][4] == 4 and plain["n"][4] == C + 3
    assert plain["sumsq"][5] == 0.0 and plain["small"][5] == 2 * C and plain["min"][5] == 0.0 == plain["max"][5]


# ------------------------------------------------------------------------------------------------ 7. reproducibility
def test_same_bits_eager_side_stream_and_graph_replay(ops, C):
    rng = np.random.default_rng(8)
    counts = [5, 300, C + 1, 40 * C + 2] + [1 + i % 50 for i in range(200)]
    tensors = [rng.standard_normal(c).astype(np.float32) for c in counts]
    flat, offsets, _ = tnp.pack(tensors)
    other = np.where(np.isfinite(flat), flat * np.float32(1.7) + np.float32(0.3), flat).astype(np.float32)
    flags, _ = _mixed_flags(flat.size, 80)
    plan = ops.TensorStatsPlan(offsets, counts, DEV)
    buf, bufb, fl = _up(flat), _up(0.5 * other), _up(flags)

    def eager(contents):
        buf.copy_(_up(contents))
        out = ops.tensor_stats(plan, buf, bufb, fl, 0.1)
        assert out.data_ptr() == plan.records.data_ptr()
        return ops.tensor_stats_records(out).tobytes()

    first, second = eager(flat), eager(flat)
    assert first == second
    want_other = eager(other)
    assert want_other != first
    side = torch.cuda.Stream()
    buf.copy_(_up(flat))
    plan.records.zero_()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.tensor_stats(plan, buf, bufb, fl, 0.1)
    torch.cuda.current_stream().wait_stream(side)
    assert ops.tensor_stats_records(plan.records).tobytes() == first
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.tensor_stats(plan, buf, bufb, fl, 0.1)
    for contents, want in ((other, want_other), (flat, first)):
        buf.copy_(_up(contents))
        plan.records.zero_()
        g.replay()
        assert ops.tensor_stats_records(plan.records).tobytes() == want


def test_latch_kernel(ops):
    """Clean records: not a byte is written.  Offenders: all records are copied, the state names the first and the last and counts them;
    a second event overwrites the first.  300 tensors: more than one pass of the 256 lanes."""
    n = 300
    recs = np.zeros(n, ops.TENSOR_STATS_RECORD)
    recs["sum"] = np.arange(n)
    records, latched = _up(recs.view(np.uint8)), torch.full((64 * n,), 0xAB, dtype=torch.uint8, device=DEV)
    state = torch.tensor([0, -5, -6, -7], dtype=torch.int32, device=DEV)
    ops.tensor_stats_latch(records, n, latched, state)
    assert state.tolist() == [0, -5, -6, -7] and (latched == 0xAB).all()
    for event, bad in ((1, {257: 3, 12: 1, 299: 2}), (2, {0: 9}), (3, {299: 1})):
        recs["nonfinite"] = 0
        for t, k in bad.items():
            recs["nonfinite"][t] = k
        records.copy_(_up(recs.view(np.uint8)))
        ops.tensor_stats_latch(records, n, latched, state)
        assert state.tolist() == [event, min(bad), max(bad), len(bad)]
        assert latched.cpu().numpy().tobytes() == recs.tobytes()
    recs["nonfinite"] = 0
    records.copy_(_up(recs.view(np.uint8)))
    keep = latched.clone()
    ops.tensor_stats_latch(records, n, latched, state)
    assert state.tolist() == [3, 299, 299, 1] and torch.equal(latched, keep)


# ------------------------------------------------------------------------------------------------ 8. FlatAdamW
def _check_derived(got, want, scale=1.0):
    """A tensor_stats entry against derive_tensor_stats' formulas on the restatement's record, with the summation bounds carried through
    them: B_s, B_q on the sums, a few float64 roundings (8 x 2^-53 relative) on top."""
    m = want["n"] - want["nonfinite"]
    assert (got["numel"], got["nonfinite"], got["small"]) == (want["n"], want["nonfinite"], want["small"])
    if m == 0:
        assert math.isnan(got["mean"]) and math.isnan(got["std"]) and got["norm"] == 0.0
        return
    s, u = abs(scale), 8 * 2.0 ** -53
    assert got["min"] == float(want["min"]) * scale and got["max"] == float(want["max"]) * scale
    assert got["abs_max"] == max(abs(float(want["min"])), abs(float(want["max"]))) * s
    b_s, b_q = tnp.sum_bound(m, want["sumabs"]), tnp.sum_bound(m, want["sumsq"])
    mean = want["sum"] / m
    assert abs(got["mean"] - mean * scale) <= s * (b_s / m + u * abs(mean))
    assert abs(got["abs_mean"] - s * want["sumabs"] / m) <= s * (b_s / m + u * want["sumabs"] / m)
    assert abs(got["norm"] ** 2 - s * s * want["sumsq"]) <= s * s * (b_q + u * want["sumsq"])
    var = max(want["sumsq"] / m - mean * mean, 0.0)
    if want["min"] == want["max"]:
        assert got["std"] == 0.0
    else:
        assert abs(got["std"] ** 2 - s * s * var) <= s * s * (b_q / m + 2 * abs(mean) * b_s / m + (b_s / m) ** 2 + u * want["sumsq"] / m)


def _small_model():
    """conv / BatchNorm / Linear with odd sizes (135, 5, 5, 5, 315, 7 elements: padding behind all but one) and a Linear that never
    receives a gradient.  Forward and backward run on the host: the gradients are torch's."""
    torch.manual_seed(4)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.ReLU(), torch.nn.Flatten(),
                            torch.nn.Linear(45, 7))
    m.add_module("dead", torch.nn.Linear(3, 3))
    x = torch.randn(6, 3, 5, 5)
    (m[4](m[3](m[2](m[1](m[0](x))))) ** 2).mean().backward()
    grads = {n: (None if p.grad is None else p.grad.detach().numpy().copy()) for n, p in m.named_parameters()}
    return m.to(DEV), grads


def test_flat_adamw_statistics_update_and_latch(ops):
    from infantposeestimation_gaussianbias_amd import engine
    m, grads = _small_model()
    opt = engine.FlatAdamW(m, lr=1e-2, skip_nonfinite=True, trace_nonfinite=True)
    assert any(o % 4 == 0 and p.numel() % 4 for o, p in zip(opt.offsets, opt.params))
    opt.snapshot_params()
    before = opt.flat.cpu().numpy().copy()
    opt.step(grad_scale=0.5)                                     # adopts torch's gradients; "dead.*" turn inactive
    assert opt.nonfinite_trace() is None and opt.trace_state.tolist() == [0, 0, 0, 0] and not opt.trace_latched.any()
    # gradients, as the update saw them (scale) and raw
    for scale in (1.0, 0.5):
        st = opt.tensor_stats("grad", tiny=1e-6, scale=scale)
        assert list(st) == opt.names
        for n, d in st.items():
            if grads[n] is None:
                assert d["numel"] == 0 and math.isnan(d["mean"]) and n.startswith("dead")
            else:
                _check_derived(d, tnp.record_np(grads[n], tiny=1e-6), scale)
    raw = ops.tensor_stats_records(ops.tensor_stats(opt._stats_plan, opt.grad, flags=opt.flags))
    total = math.sqrt(math.fsum(float(r["sumsq"]) for r in raw)) * 0.5
    gs = opt.guard_stats()
    assert gs["skipped_last"] == 0 and abs(gs["grad_norm"] - total) <= 2.0 ** -23 * total, (gs, total)
    # the update against the snapshot
    after = opt.flat.cpu().numpy().copy()
    st = opt.tensor_stats("update")
    for n, p, o in zip(opt.names, opt.params, opt.offsets):
        k = p.numel()
        if grads[n] is None:
            assert st[n]["numel"] == 0 and np.array_equal(after[o:o + k], before[o:o + k])
        else:
            _check_derived(st[n], tnp.record_np(after[o:o + k] - before[o:o + k]))
    assert st["0.weight"]["norm"] > 0 and st["4.weight"]["norm"] > 0
    ratio = engine.update_to_weight_ratio(st, opt.tensor_stats("param"))
    # one step of lr 1e-2 on weights of order 0.1 .. 1; BatchNorm's bias started at 0, so it IS its update
    assert all(0 <= ratio[n] <= 1 for n in opt.names if grads[n] is not None) and 0 < ratio["4.weight"] < 0.5 and ratio["1.bias"] == 1.0
    assert math.isnan(ratio["dead.weight"]) or ratio["dead.weight"] == 0.0
    # the latch
    mid, other = opt.names.index("1.weight"), opt.names.index("4.weight")
    view = opt.grad_view(mid)
    keep = view.clone()
    view.reshape(-1)[2] = float("inf")
    masters = opt.flat.clone()
    opt.step(grad_scale=0.5)
    tr = opt.nonfinite_trace()
    assert tr == {"events": 1, "tensors": {"1.weight": 1}, "first": "1.weight", "last": "1.weight"}
    assert opt.guard_stats()["skipped_last"] == 1 and torch.equal(opt.flat.view(torch.int32), masters.view(torch.int32))
    view.copy_(keep)
    latched, state = opt.trace_latched.clone(), opt.trace_state.clone()
    opt.step(grad_scale=0.5)
    assert opt.guard_stats()["skipped_last"] == 0 and not torch.equal(opt.flat, masters)
    assert torch.equal(opt.trace_latched, latched) and torch.equal(opt.trace_state, state)
    opt.grad_view(other).reshape(-1)[[0, 314]] = float("nan")
    opt.step(grad_scale=0.5)
    tr = opt.nonfinite_trace()
    assert tr == {"events": 2, "tensors": {"4.weight": 2}, "first": "4.weight", "last": "4.weight"}
    assert not torch.equal(opt.trace_latched, latched)
    # the latched records are the whole step's: the clean tensors' statistics are in them too
    rec = ops.tensor_stats_records(opt.trace_latched)
    assert rec["n"][other] == 315 and rec["n"][mid] == 5 and rec["nonfinite"][mid] == 0 and rec["sumsq"][mid] > 0


def test_flat_adamw_other_buffers_and_against(ops):
    """The moments, the EMA, and `against`: ema - flat is the difference mode on the two buffers, checked against the fp32 difference
    taken on the host."""
    from infantposeestimation_gaussianbias_amd import engine
    m, grads = _small_model()
    opt = engine.FlatAdamW(m, lr=1e-2, ema_decay=0.9)
    for _ in range(3):
        opt.step()
    host = {k: getattr(opt, k).cpu().numpy() for k in ("flat", "exp_avg", "exp_avg_sq", "ema")}
    cases = {("exp_avg", None): host["exp_avg"], ("exp_avg_sq", None): host["exp_avg_sq"], ("ema", None): host["ema"],
             ("param", None): host["flat"], ("ema", "param"): host["ema"] - host["flat"], ("param", "ema"): host["flat"] - host["ema"]}
    for (which, against), want in cases.items():
        st = opt.tensor_stats(which, against=against, tiny=1e-4)
        for n, p, o in zip(opt.names, opt.params, opt.offsets):
            if grads[n] is None:
                assert st[n]["numel"] == 0
            else:
                _check_derived(st[n], tnp.record_np(want[o:o + p.numel()], tiny=1e-4))
    assert opt.tensor_stats("ema", against="param")["4.weight"]["norm"] > 0
    assert opt.tensor_stats("exp_avg_sq")["4.weight"]["min"] >= 0


def test_public_functions_on_a_model(ops):
    from infantposeestimation_gaussianbias_amd import utils
    m, grads = _small_model()
    gs = utils.gradient_statistics(m)
    assert list(gs) == [n for n in grads if grads[n] is not None]
    for n, d in gs.items():
        _check_derived(d, tnp.record_np(grads[n]))
        assert {"mean", "std", "min", "max", "norm"} <= set(d)
    names, ave, mx = utils.gradient_flow(m.named_parameters())
    assert names == list(gs) and ave == [gs[n]["abs_mean"] for n in names] and mx == [gs[n]["abs_max"] for n in names]
    ws = utils.weight_statistics(m)
    weights = {n: p.detach().cpu().numpy().reshape(-1) for n, p in m.named_parameters() if "weight" in n}
    assert list(ws["layers"]) == list(weights) and list(ws["sparsity"]) == list(utils.tensor_stats.DEFAULT_THRESHOLDS)
    allw = np.concatenate(list(weights.values())).astype(np.float64)
    for level, share in ws["sparsity"].items():
        assert share == (np.abs(allw) < level).sum() / allw.size, level          # the reference's expression
    assert 0 < ws["sparsity"][1e-1] < 1
    for n, w in weights.items():
        _check_derived({**ws["layers"][n], "small": 0}, tnp.record_np(w))
    ts = utils.tensor_statistics([("a", torch.arange(6, device=DEV, dtype=torch.float32).reshape(2, 3)),
                                  ("b", torch.tensor([1.0, float("nan")], device=DEV))], tiny=1.0)
    assert (ts["a"]["mean"], ts["a"]["min"], ts["a"]["max"], ts["a"]["small"], ts["a"]["numel"]) == (2.5, 0.0, 5.0, 2, 6)
    assert (ts["b"]["nonfinite"], ts["b"]["mean"], ts["b"]["std"]) == (1, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ 9. Trainer, graph mode
def _setup():
    """The fixture of test_gpu_ema.py: hrformer_small, 96 x 128, B = 4."""
    from infantposeestimation_gaussianbias_amd.configs import get_config
    from infantposeestimation_gaussianbias_amd.datasets import synthetic_batch
    cfg = get_config("hrformer_small")
    cfg.data.input_size, cfg.data.heatmap_size = (96, 128), (24, 32)
    batches = [synthetic_batch(4, cfg.data.input_size, cfg.data.heatmap_size, 17, 2.0, DEV, seed=30 + i) for i in range(3)]
    return cfg, batches


def _trainer(cfg, **kw):
    from infantposeestimation_gaussianbias_amd import engine
    from infantposeestimation_gaussianbias_amd.models import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV)
    model.backbone.drop_path_rate = 0.0
    return engine.Trainer(model, cfg, iters_per_epoch=2, use_graph=True, graph_warmup=2, **kw)


def _poisoned(batch):
    """One NaN in `target` (test_gpu_grad_guard.py): the forward stays finite, the loss and every gradient turn NaN."""
    bad = dict(batch)
    bad["target"] = bad["target"].clone()
    b, k = (bad["target_weight"].reshape(4, 17) > 0).nonzero()[0].tolist()
    bad["target"][b, k, 3, 5] = float("nan")
    return bad


def test_trainer_graph_mode_trace_and_statistics(ops):
    """Seven steps, the fifth (a replay) poisoned: the latch inside the captured step records it and nothing else; the run's masters are
    bitwise those of a trainer without skip_nonfinite / trace_nonfinite over the six clean batches (whose schedule is ticked once
    where the skipped step was: the learning rate advances on skipped steps too); and the statistics of a replayed step's gradients
    are those of the gradient buffer copied to the host."""
    cfg, batches = _setup()
    seq = [batches[i % 3] for i in range(4)] + [_poisoned(batches[4 % 3])] + [batches[5 % 3], batches[6 % 3]]
    tr = _trainer(cfg, skip_nonfinite=True, trace_nonfinite=True)
    opt = tr.opt
    for b in seq[:4]:
        tr.step(b)
        assert opt.nonfinite_trace() is None
    assert tr._graph is not None and tr._graph_has_opt
    tr.step(seq[4])
    trace = opt.nonfinite_trace()
    active = [n for n, a in zip(opt.names, opt.active) if a]
    assert 0 < len(active) < len(opt.names)
    # what the trace must say, counted on the host from the gradient buffer the skipped step left behind
    g, fl = opt.grad.cpu().numpy(), opt.flags.cpu().numpy()
    want = {}
    for n, p, o in zip(opt.names, opt.params, opt.offsets):
        k = tnp.record_np(g[o:o + p.numel()], fl[o:o + p.numel()])["nonfinite"]
        if k:
            want[n] = k
    assert trace["events"] == 1 and dict(trace["tensors"]) == want and list(trace["tensors"]) == list(want)
    assert trace["first"] == next(iter(want)) and trace["last"] == list(want)[-1]
    # the poison reaches every gradient that the heatmap target reaches: the whole backbone and the heatmap head.  (Not literally every
    # active tensor: the loss terms of the head's other branches do not read `target`, and ten tensors of theirs stay finite.)
    assert set(want) <= set(active) and len(want) >= 0.9 * len(active)
    assert all(n in want for n in active if n.startswith("backbone."))
    assert opt.guard_stats()["skipped_steps"] == 1
    tr.step(seq[5], snapshot=True)
    assert opt.nonfinite_trace() == trace
    upd = opt.tensor_stats("update")
    assert all((upd[n]["numel"] > 0) == a and (a or upd[n]["norm"] == 0) for n, a in zip(opt.names, opt.active))
    assert sum(upd[n]["norm"] > 0 for n in active) >= 0.9 * len(active)
    tr.step(seq[6])
    torch.cuda.synchronize()
    assert opt.nonfinite_trace() == trace and opt.guard_stats()["skipped_steps"] == 1 and int(opt.step_dev) == 6
    # statistics of the replayed step's gradients: still in the buffer
    st = opt.tensor_stats("grad", tiny=1e-8)
    g = opt.grad.cpu().numpy()
    raw = ops.tensor_stats_records(opt._stats_plan.records)
    for i, (n, p, o) in enumerate(zip(opt.names, opt.params, opt.offsets)):
        want = tnp.record_np(g[o:o + p.numel()], fl[o:o + p.numel()], 1e-8)
        _check(raw[i], want, n)
        assert st[n] == ops.derive_tensor_stats(raw[i]) or not opt.active[i]
        assert (st[n]["numel"] == p.numel()) if opt.active[i] else (st[n]["numel"] == 0)
    total = math.sqrt(math.fsum(float(r["sumsq"]) for r in raw))
    assert abs(opt.guard_stats()["grad_norm"] - total) <= 2.0 ** -23 * total

    plain = _trainer(cfg)
    assert not plain.opt.guarded and not plain.opt.trace_nonfinite and plain.opt._stats_plan is None
    for i, b in enumerate(seq):
        if i == 4:
            plain.sched.step()
        else:
            plain.step(b)
    torch.cuda.synchronize()
    assert plain._graph is not None and plain.opt._stats_plan is None and plain.opt.snapshot is None
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(opt, name).view(torch.int32), getattr(plain.opt, name).view(torch.int32)), name
