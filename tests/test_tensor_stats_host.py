"""Host-side checks of the per-tensor statistics (no GPU): the derived values against numpy on exact records, the launch plan
(every element covered once, nothing in the padding, counts match the queries), the header's entries and their argument checks (which
run before any device is touched), the scripts' flags, and the engine's defaults: no buffers, and the methods that need an option
say so."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tensor_stats_np as tnp

TENSOR_ROW = np.dtype([("first_item", "<i4"), ("n_items", "<i4"), ("zero", "<i8")])
ITEM_ROW = np.dtype([("start", "<i8"), ("count", "<i4"), ("tensor", "<i4")])


@pytest.fixture(scope="module")
def ops():
    from infantposeestimation_gaussianbias_amd import hipops
    return hipops


def _close(got, want, tol=1e-9):
    return abs(got - want) <= tol * abs(want)


# ------------------------------------------------------------------------------------------------ derived values
@pytest.mark.parametrize("n, loc, scale", [(1, 0.3, 1.0), (7, 0.0, 1.0), (257, 0.5, 2.0), (5000, -3.0, 0.1), (4096, 0.0, 1e-6)])
def test_derived_values_match_numpy(ops, n, loc, scale):
    """Well-conditioned tensors (|mean| <= 30 std, so E[x^2] - mean^2 loses at most three digits of sixteen): 1e-9 relative covers the
    handful of float64 operations on exactly summed records."""
    rng = np.random.default_rng(n)
    x = (loc + scale * rng.standard_normal(n)).astype(np.float32)
    d = ops.derive_tensor_stats(tnp.record_np(x))
    x64 = x.astype(np.float64)
    assert _close(d["mean"], np.mean(x64)) or (n == 1 and d["mean"] == x64[0])
    assert d["min"] == np.min(x64) and d["max"] == np.max(x64)
    assert _close(d["norm"], np.linalg.norm(x64)) and _close(d["abs_mean"], np.abs(x64).mean()) and d["abs_max"] == np.abs(x64).max()
    assert (d["std"] == 0.0 if n == 1 else _close(d["std"], np.std(x64)))
    assert (d["numel"], d["nonfinite"], d["small"]) == (n, 0, 0)
    assert set(d) == {"mean", "std", "min", "max", "norm", "abs_mean", "abs_max", "numel", "nonfinite", "small"}
    assert all(type(v) in (float, int) for v in d.values())


def test_derived_values_scale_constant_and_empty(ops):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(333).astype(np.float32)
    rec = tnp.record_np(x, tiny=0.5)
    one, half, neg = ops.derive_tensor_stats(rec), ops.derive_tensor_stats(rec, 0.5), ops.derive_tensor_stats(rec, -2.0)
    for k in ("mean", "std", "min", "max", "norm", "abs_mean", "abs_max"):
        assert half[k] == 0.5 * one[k], k
    assert neg["mean"] == -2 * one["mean"] and (neg["min"], neg["max"]) == (-2 * one["max"], -2 * one["min"])
    assert neg["std"] == 2 * one["std"] and neg["norm"] == 2 * one["norm"] and neg["abs_max"] == 2 * one["abs_max"]
    assert one["small"] == half["small"] == int((np.abs(x) <= 0.5).sum()) > 0          # counts are not scaled
    # a constant tensor: E[x^2] - mean^2 is rounding noise of either sign; the answer is 0, not its square root (nor nan)
    for c, n in ((0.1, 1000), (1 / 3, 77), (-123.456, 4099), (1e-30, 5), (3e38, 3)):
        d = ops.derive_tensor_stats(tnp.record_np(np.full(n, c, np.float32)))
        assert d["std"] == 0.0 and d["mean"] == pytest.approx(float(np.float32(c)), rel=1e-15), (c, n, d)
    # nothing finite: counts stand, mean and std are nan, the norm of nothing is 0
    d = ops.derive_tensor_stats(tnp.record_np(np.array([np.nan, np.inf, -np.inf], np.float32)))
    assert (d["numel"], d["nonfinite"]) == (3, 3) and math.isnan(d["mean"]) and math.isnan(d["std"]) and d["norm"] == 0.0
    assert d["min"] == math.inf and d["max"] == -math.inf
    d = ops.derive_tensor_stats(tnp.record_np(np.ones(4, np.float32), np.zeros(4, np.uint8)))          # an inactive tensor
    assert d["numel"] == 0 and math.isnan(d["mean"])
    # inf / NaN are counted and left out
    d = ops.derive_tensor_stats(tnp.record_np(np.array([1, np.nan, 3, np.inf], np.float32)))
    assert (d["numel"], d["nonfinite"], d["mean"], d["std"], d["max"]) == (4, 2, 2.0, 1.0, 3.0)


def test_record_dtype_is_the_documented_layout(ops):
    dt = ops.TENSOR_STATS_RECORD
    assert dt.itemsize == 64 and dt.names == tnp.FIELDS
    assert [dt.fields[k][1] for k in dt.names] == [0, 8, 16, 24, 28, 32, 40, 48, 56]
    assert [dt.fields[k][0].str for k in dt.names] == ["<f8", "<f8", "<f8", "<f4", "<f4", "<i8", "<i8", "<i8", "<i8"]


# ------------------------------------------------------------------------------------------------ plan
def _split(plan, n_tensors, n_items):
    return plan[:16 * n_tensors].view(TENSOR_ROW), plan[16 * n_tensors:].view(ITEM_ROW)


def test_plan_covers_every_element_once_and_no_padding(ops):
    from infantposeestimation_gaussianbias_amd import _lib
    C = ops.tensor_stats_chunk_elems()
    assert C >= 256 and C % 256 == 0
    rng = np.random.default_rng(11)
    counts = [1, 2, 3, 4, 5, 255, 256, 257, C - 1, C, C + 1, 2 * C, 2 * C + 1, 7 * C + 3] + rng.integers(1, 3 * C, 40).tolist()
    offsets, off = [], 8                                   # the table need not start at 0, nor be packed tightly
    for c in counts:
        offsets.append(off)
        off += -(-c // 4) * 4 + 4 * int(rng.integers(0, 3))
    plan, n_items = ops.tensor_stats_plan_host(offsets, counts)
    assert n_items == sum(-(-c // C) for c in counts)
    assert plan.nbytes == _lib.lib.pk_tensor_stats_plan_bytes(n_items, len(counts)) == 16 * (len(counts) + n_items)
    assert _lib.lib.pk_tensor_stats_ws_bytes(n_items, len(counts)) == 64 * n_items
    rows, items = _split(plan, len(counts), n_items)
    assert len(items) == n_items and (rows["zero"] == 0).all()
    seen = np.zeros(off, np.int32)
    for t, (o, c) in enumerate(zip(offsets, counts)):
        mine = items[rows["first_item"][t]:rows["first_item"][t] + rows["n_items"][t]]
        assert rows["n_items"][t] == -(-c // C) and (mine["tensor"] == t).all()
        assert (mine["start"] % 4 == 0).all() and (mine["count"] >= 1).all() and (mine["count"] <= C).all()
        assert (mine["count"][:-1] == C).all()                                   # only a tensor's last item is short
        assert mine["start"][0] == o and (np.diff(mine["start"]) == C).all() and mine["count"].sum() == c
        for s, k in zip(mine["start"], mine["count"]):
            assert o <= s and s + k <= o + c                                     # never into the padding
            seen[s:s + k] += 1
    owned = np.zeros(off, bool)
    for o, c in zip(offsets, counts):
        owned[o:o + c] = True
    assert np.array_equal(seen, owned.astype(np.int32))
    assert np.array_equal(np.sort(rows["first_item"]), rows["first_item"]) and rows["first_item"][0] == 0
    # the same table gives the same plan
    assert np.array_equal(plan, ops.tensor_stats_plan_host(offsets, counts)[0])


# ------------------------------------------------------------------------------------------------ header, library, argument checks
def _aligned(n_bytes):
    raw = np.zeros(n_bytes + 16, np.uint8)
    return raw, raw.ctypes.data + (-raw.ctypes.data) % 16


def test_header_declares_the_entries():
    from infantposeestimation_gaussianbias_amd import _lib
    decl = _lib.declared_symbols()
    want = {"pk_tensor_stats_chunk_elems": 0, "pk_tensor_stats_plan": 4, "pk_tensor_stats_plan_bytes": 2, "pk_tensor_stats_ws_bytes": 2,
            "pk_tensor_stats": 11, "pk_tensor_stats_latch": 5}
    for name, n_args in want.items():
        assert name in decl and hasattr(_lib.lib, name) and len(decl[name][1]) == n_args, name
    assert _lib.CONSTANTS["PK_TENSOR_STATS_RECORD_BYTES"] == 64
    assert decl["pk_tensor_stats"][1][6] is ctypes.c_float and decl["pk_tensor_stats"][1][8] is ctypes.c_int64


def test_arguments_are_checked_before_any_device_is_touched():
    """Every refusal names its function.  All pointers are host pointers: nothing may be launched, and nothing is."""
    from infantposeestimation_gaussianbias_amd import _lib
    L = _lib.lib

    def rejected(rc, who, word):
        msg = L.pk_last_error_string()
        assert rc < 0 and who in msg and word in msg, (rc, msg)

    # queries
    for q in (L.pk_tensor_stats_plan_bytes, L.pk_tensor_stats_ws_bytes):
        name = b"pk_tensor_stats_plan_bytes" if q is L.pk_tensor_stats_plan_bytes else b"pk_tensor_stats_ws_bytes"
        rejected(q(0, 0), name, b"n_tensors")
        rejected(q(3, 4), name, b"n_items")              # fewer items than tensors
        rejected(q(1 << 30, 1), name, b"n_items")
        assert q(4, 3) > 0
    # plan
    seg = np.array([[0, 5], [8, 3000], [3008, 1]], np.int64)
    n_items = L.pk_tensor_stats_plan(seg.ctypes.data, 3, None, 0)
    assert n_items == 4 if L.pk_tensor_stats_chunk_elems() == 2048 else n_items >= 3
    need = L.pk_tensor_stats_plan_bytes(n_items, 3)
    keep, out = _aligned(need)
    assert L.pk_tensor_stats_plan(seg.ctypes.data, 3, out, need) == n_items
    rejected(L.pk_tensor_stats_plan(seg.ctypes.data, 3, out, need - 1), b"pk_tensor_stats_plan", b"capacity")
    rejected(L.pk_tensor_stats_plan(None, 3, out, need), b"pk_tensor_stats_plan", b"null")
    rejected(L.pk_tensor_stats_plan(seg.ctypes.data, 0, out, need), b"pk_tensor_stats_plan", b"n_tensors")
    for bad_row, word in (((6, 5), b"multiple of 4"), ((-4, 5), b"multiple of 4"), ((8, 0), b"count"), ((8, -1), b"count")):
        bad = seg.copy()
        bad[1] = bad_row
        rejected(L.pk_tensor_stats_plan(bad.ctypes.data, 3, None, 0), b"pk_tensor_stats_plan", word)
        rejected(L.pk_tensor_stats_plan(bad.ctypes.data, 3, out, need), b"pk_tensor_stats_plan", word)
    # launcher
    bufs = [_aligned(4096) for _ in range(6)]
    a, b, fl, plan, ws, rec = (p for _, p in bufs)
    ws_bytes = L.pk_tensor_stats_ws_bytes(n_items, 3)

    def run(a=a, b=b, fl=fl, plan=plan, nt=3, ni=n_items, tiny=0.0, ws=ws, wsb=ws_bytes, rec=rec):
        return L.pk_tensor_stats(a, b, fl, plan, nt, ni, tiny, ws, wsb, rec, None)

    who = b"pk_tensor_stats:"
    for kw in ({"a": None}, {"plan": None}, {"ws": None}, {"rec": None}):
        rejected(run(**kw), who, b"null")
    for kw in ({"a": a + 4}, {"b": b + 8}, {"fl": fl + 2}, {"plan": plan + 8}, {"ws": ws + 8}, {"rec": rec + 4}):
        rejected(run(**kw), who, b"misaligned")
    for bad in (-1e-30, -1.0, float("nan"), float("inf"), -float("inf")):
        rejected(run(tiny=bad), who, b"tiny")
    rejected(run(wsb=ws_bytes - 1), who, b"ws_bytes")
    rejected(run(nt=0), who, b"n_tensors")
    rejected(run(ni=2), who, b"n_items")
    # latch
    st_keep, st = _aligned(16)
    who = b"pk_tensor_stats_latch"
    rejected(L.pk_tensor_stats_latch(None, 3, ws, st, None), who, b"null")
    rejected(L.pk_tensor_stats_latch(rec, 3, None, st, None), who, b"null")
    rejected(L.pk_tensor_stats_latch(rec, 3, ws, None, None), who, b"null")
    rejected(L.pk_tensor_stats_latch(rec + 8, 3, ws, st, None), who, b"misaligned")
    rejected(L.pk_tensor_stats_latch(rec, 3, ws + 4, st, None), who, b"misaligned")
    rejected(L.pk_tensor_stats_latch(rec, 3, ws, st + 2, None), who, b"misaligned")
    rejected(L.pk_tensor_stats_latch(rec, 0, ws, st, None), who, b"n_tensors")
    rejected(L.pk_tensor_stats_latch(rec, 3, rec, st, None), who, b"of its own")
    del keep, bufs, st_keep


def test_ops_refuse_cpu_tensors(ops):
    from infantposeestimation_gaussianbias_amd import _lib, utils
    plan = ops.TensorStatsPlan([0, 8], [5, 3], "cpu")
    assert (plan.n_tensors, plan.n_items, plan.extent) == (2, 2, 11)
    with pytest.raises(_lib.PoseKernelError, match="CUDA"):
        ops.tensor_stats(plan, torch.zeros(12))
    with pytest.raises(_lib.PoseKernelError, match="CUDA"):
        ops.tensor_stats_latch(plan.records, 2, torch.zeros_like(plan.records), torch.zeros(4, dtype=torch.int32))
    m = torch.nn.Linear(3, 2)
    m(torch.ones(1, 3)).sum().backward()
    for fn in (lambda: utils.tensor_statistics([("w", m.weight.data)]), lambda: utils.gradient_statistics(m),
               lambda: utils.gradient_flow(m.named_parameters()), lambda: utils.weight_statistics(m)):
        with pytest.raises(_lib.PoseKernelError, match="CUDA"):
            fn()
    for name in ("tensor_statistics", "gradient_statistics", "gradient_flow", "weight_statistics"):
        assert name in utils.__all__ and callable(getattr(utils, name))


def test_sparsity_threshold_turns_less_than_into_at_most():
    """The reference counts |w| < level; the record counts |x| <= tiny: tiny is the largest float32 below the level."""
    from infantposeestimation_gaussianbias_amd.utils import tensor_stats as ts
    for level in ts.DEFAULT_THRESHOLDS + (0.5, 1.0, 2.0 ** -20):
        t = np.float32(ts._below(level))
        assert float(t) < level <= float(np.nextafter(t, np.float32(np.inf))), level


# ------------------------------------------------------------------------------------------------ scripts
def test_parsers_have_both_flags_off_by_default():
    import train
    p = train.build_parser()
    a = p.parse_args([])
    assert a.tensor_stats == 0 and a.trace_nonfinite is False
    a = p.parse_args(["--graph", "--tensor_stats", "5", "--trace_nonfinite", "--skip_nonfinite"])
    assert a.tensor_stats == 5 and a.trace_nonfinite is True and a.skip_nonfinite and a.graph


def test_report_lines_of_the_training_script():
    import train

    class Opt:
        def __init__(self, tr):
            self.tr = tr

        def nonfinite_trace(self):
            return self.tr

    assert train.nonfinite_report(Opt(None), 0) == (None, 0)
    tr = {"events": 3, "tensors": {"a.weight": 2, "head.bias": 7}, "first": "a.weight", "last": "head.bias"}
    line, seen = train.nonfinite_report(Opt(tr), 1)
    assert seen == 3 and "2 step(s)" in line and "2 tensors" in line and "head.bias (7 elements)" in line
    assert train.nonfinite_report(Opt(tr), 3) == (None, 3)


# ------------------------------------------------------------------------------------------------ engine
def _model():
    torch.manual_seed(1)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3))


def test_flat_adamw_defaults_have_no_statistics_buffers():
    from infantposeestimation_gaussianbias_amd import engine, hipops
    for kw in ({}, {"trace_nonfinite": False}, {"skip_nonfinite": True}, {"ema_decay": 0.9}):
        opt = engine.FlatAdamW(_model(), **kw)
        assert opt.trace_nonfinite is False and opt._stats_plan is None and opt.snapshot is None
        assert not any(hasattr(opt, a) for a in ("trace_records", "trace_latched", "trace_state"))
        with pytest.raises(RuntimeError, match="trace is off"):
            opt.nonfinite_trace()
    assert hipops.GUARD_STATE_WORDS == 4 and hipops.LATCH_STATE_WORDS == 4
    import inspect
    assert inspect.signature(engine.FlatAdamW.__init__).parameters["trace_nonfinite"].default is False
    assert inspect.signature(engine.Trainer.__init__).parameters["trace_nonfinite"].default is False
    assert inspect.signature(engine.Trainer.step).parameters["snapshot"].default is False


def test_methods_that_need_an_option_say_so():
    from infantposeestimation_gaussianbias_amd import engine
    opt = engine.FlatAdamW(_model())
    with pytest.raises(RuntimeError, match=r"tensor_stats: the weight EMA is off \(ema_decay=0\)"):
        opt.tensor_stats("ema")
    with pytest.raises(RuntimeError, match="EMA is off"):
        opt.tensor_stats("param", against="ema")
    with pytest.raises(RuntimeError, match="snapshot"):
        opt.tensor_stats("update")
    with pytest.raises(ValueError, match="unknown buffer"):
        opt.tensor_stats("weights")
    assert opt._stats_plan is None                                  # a refused call builds nothing
    opt.snapshot_params()
    assert torch.equal(opt.snapshot, opt.flat) and opt.snapshot.data_ptr() != opt.flat.data_ptr()
    ptr = opt.snapshot.data_ptr()
    opt.flat.add_(1.0)
    opt.snapshot_params()
    assert opt.snapshot.data_ptr() == ptr and torch.equal(opt.snapshot, opt.flat)          # static: allocated once
    with pytest.raises(ValueError, match="against"):
        opt.tensor_stats("update", against="param")


def test_trace_buffers_and_empty_trace():
    """trace_nonfinite builds the static buffers at construction (a captured step holds their addresses); before any event the trace is
    None.  The plan is the one tensor_stats uses."""
    from infantposeestimation_gaussianbias_amd import engine, hipops
    opt = engine.FlatAdamW(_model(), trace_nonfinite=True)
    n = len(opt.params)
    assert not opt.guarded                                          # the trace alone does not guard the step
    assert opt._stats_plan.n_tensors == n and opt._stats_plan.offsets == opt.offsets
    assert opt._stats_plan.counts == [p.numel() for p in opt.params] and opt._stats_plan.extent <= opt.numel
    for b in (opt.trace_records, opt.trace_latched):
        assert b.dtype == torch.uint8 and b.numel() == 64 * n
    assert opt.trace_records.data_ptr() != opt._stats_plan.records.data_ptr()
    assert opt.trace_state.dtype == torch.int32 and opt.trace_state.tolist() == [0] * hipops.LATCH_STATE_WORDS
    assert opt.nonfinite_trace() is None
    # a latched event, as the device would have left it
    recs = np.zeros(n, hipops.TENSOR_STATS_RECORD)
    recs["nonfinite"][[1, 3]] = (4, 1)
    opt.trace_latched.copy_(torch.from_numpy(recs.view(np.uint8)))
    opt.trace_state.copy_(torch.tensor([2, 1, 3, 2], dtype=torch.int32))
    tr = opt.nonfinite_trace()
    assert tr == {"events": 2, "tensors": {opt.names[1]: 4, opt.names[3]: 1}, "first": opt.names[1], "last": opt.names[3]}
    assert list(tr["tensors"]) == [opt.names[1], opt.names[3]]


def test_update_to_weight_ratio():
    from infantposeestimation_gaussianbias_amd import engine
    upd = {"a": {"norm": 0.5}, "b": {"norm": 0.0}, "c": {"norm": 1.0}}
    par = {"a": {"norm": 2.0}, "b": {"norm": 4.0}, "c": {"norm": 0.0}}
    r = engine.update_to_weight_ratio(upd, par)
    assert list(r) == ["a", "b", "c"] and r["a"] == 0.25 and r["b"] == 0.0 and math.isnan(r["c"])
