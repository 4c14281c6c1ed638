"""Activation statistics without a GPU: the entries in the header and every refusal with its text and rank, the split of rows over
workgroups at its boundaries, the restatement against plain numpy, the bin rule over all 65 536 bf16 patterns, and the argument checks of
`activation_report`.  The launches themselves raise without a device, so nothing here goes past an argument check."""
import math

import numpy as np
import pytest
import torch

import activation_np as anp


def _lib():
    from infantposeestimation_gaussianbias_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ C-ABI
def test_the_entries_are_declared_with_their_argument_counts():
    L = _lib()
    decl = L.declared_symbols()
    for name, n_args in (("pk_activation_stats", 10), ("pk_activation_quantiles", 11), ("pk_activation_stats_blocks", 2),
                         ("pk_activation_stats_slab", 1), ("pk_activation_stats_ws_bytes", 2), ("pk_activation_quantiles_ws_bytes", 2)):
        assert name in decl and len(decl[name][1]) == n_args and hasattr(L.lib, name), name
    want = {"PK_ACT_RECORD_BYTES": 64, "PK_ACT_HIST_BINS": 4096, "PK_ACT_MAX_CHANNELS": 2048, "PK_ACT_MAX_QUANTILES": 16,
            "PK_ACT_MAX_ELEMS": 2 ** 38}
    assert {k: L.CONSTANTS.get(k) for k in want} == want
    from infantposeestimation_gaussianbias_amd import hipops
    assert hipops.ACT_RECORD.itemsize == 64 and hipops.ACT_RECORD == anp.RECORD


def test_every_refusal_comes_back_with_its_text_and_in_its_rank():
    L = _lib().lib
    p = 64                                                        # a non-null, 16-byte aligned pointer value that is never dereferenced
    err = lambda: L.pk_last_error_string().decode()
    q_ok = np.array([0.25, 0.5], np.float64)

    def stats(x=p, M=100, C=24, c_used=24, ws=p, ws_bytes=1 << 30, records=p, hist=p):
        return L.pk_activation_stats(x, M, C, c_used, ws, ws_bytes, records, hist, 0, None)

    def quant(x=p, M=100, C=24, c_used=24, hist=p, q=q_ok, Q=2, ws=p, ws_bytes=1 << 30, order=p):
        return L.pk_activation_quantiles(x, M, C, c_used, hist, None if q is None else q.ctypes.data, Q, ws, ws_bytes, order, None)

    for name in ("x", "ws", "records", "hist"):
        assert stats(**{name: None}) == -1 and err() == "pk_activation_stats: null pointer", name
    for name in ("x", "hist", "q", "ws", "order"):
        assert quant(**{name: None}) == -1 and err() == "pk_activation_quantiles: null pointer", name
    for fn, who in ((stats, "pk_activation_stats"), (quant, "pk_activation_quantiles")):
        assert fn(C=20) == -1 and err() == f"{who}: C=20 must be a multiple of 8 (16-byte bf16 chunks)"
        assert fn(C=0) == -1 and err() == f"{who}: C=0 outside [8, 2048]"
        assert fn(C=2056, c_used=8) == -1 and err() == f"{who}: C=2056 outside [8, 2048]"
        assert fn(c_used=0) == -1 and err() == f"{who}: c_used=0 outside [1, C=24]"
        assert fn(c_used=25) == -1 and err() == f"{who}: c_used=25 outside [1, C=24]"
        assert fn(M=0) == -1 and err() == f"{who}: M=0 rows of C=24: M C outside [1, 2^38]"
        big = 2 ** 38 // 24 + 1
        assert fn(M=big) == -1 and err() == f"{who}: M={big} rows of C=24: M C outside [1, 2^38]"
        assert fn(x=72) == -1 and err().startswith(f"{who}: misaligned buffer")
    assert stats(hist=68) == -1 and err() == "pk_activation_stats: misaligned buffer (x, ws, records: 16 bytes; hist: 8)"
    assert quant(order=66) == -1 and err() == "pk_activation_quantiles: misaligned buffer (x, ws: 16 bytes; hist: 8; order: 4)"
    need = L.pk_activation_stats_ws_bytes(100, 24)
    assert stats(ws_bytes=need - 1) == -1
    assert err() == f"pk_activation_stats: ws_bytes={need - 1}, but M=100 C=24 need {need} (pk_activation_stats_ws_bytes)"
    need = L.pk_activation_quantiles_ws_bytes(100, 24)
    assert quant(ws_bytes=need - 1) == -1
    assert err() == f"pk_activation_quantiles: ws_bytes={need - 1}, but M=100 C=24 need {need} (pk_activation_quantiles_ws_bytes)"
    assert quant(Q=0) == -1 and err() == "pk_activation_quantiles: 0 quantiles (1 to 16)"
    assert quant(Q=17) == -1 and err() == "pk_activation_quantiles: 17 quantiles (1 to 16)"
    assert quant(q=np.array([0.5, 1.5])) == -1 and err() == "pk_activation_quantiles: q[1]=1.5 outside [0, 1]"
    assert quant(q=np.array([-0.25, 0.5])) == -1 and err() == "pk_activation_quantiles: q[0]=-0.25 outside [0, 1]"
    assert quant(q=np.array([0.5, np.nan])) == -1 and err() == "pk_activation_quantiles: q[1]=nan outside [0, 1]"
    # pairs of faults: the documented rank -- null, C % 8, range of C, c_used, M C, Q, q, alignment, workspace
    assert stats(x=None, C=20) == -1 and err() == "pk_activation_stats: null pointer"
    assert stats(C=20, c_used=0) == -1 and "multiple of 8" in err()
    assert stats(C=4096, c_used=0) == -1 and "outside [8, 2048]" in err()
    assert stats(c_used=0, M=0) == -1 and "c_used=0" in err()
    assert stats(M=0, x=72) == -1 and "M C outside" in err()
    assert stats(x=72, ws_bytes=0) == -1 and "misaligned" in err()
    assert quant(M=0, Q=0) == -1 and "M C outside" in err()
    assert quant(Q=17, q=np.array([2.0])) == -1 and "17 quantiles" in err()
    assert quant(q=np.array([2.0, 0.5]), x=72) == -1 and "q[0]=2" in err()
    assert quant(x=72, ws_bytes=0) == -1 and "misaligned" in err()


def test_split_of_rows_at_its_boundaries_and_the_workspace_queries():
    L = _lib().lib
    err = lambda: L.pk_last_error_string().decode()
    for C in (8, 24, 40, 264, 2048):
        G = 256 // (C // 8)
        slab = L.pk_activation_stats_slab(C)
        assert slab == 4 * G == anp.split(1, C)[2]
        full = 512 * slab                                         # the largest M at which every workgroup takes one slab
        for M in (1, slab - 1, slab, slab + 1, 2 * slab, full - 1, full, full + 1, 10 * full + 3, 2 ** 38 // C):
            B = L.pk_activation_stats_blocks(M, C)
            assert B == min(512, -(-M // slab)) == anp.split(M, C)[0], (M, C)
            assert L.pk_activation_stats_ws_bytes(M, C) == B * (36 * C + 4 * 4100), (M, C)
            assert L.pk_activation_quantiles_ws_bytes(M, C) == 16 * 32 + B * 4 * (32 * 16 + 4), (M, C)
    assert L.pk_activation_stats_blocks(1, 8) == 1 and L.pk_activation_stats_ws_bytes(1, 8) == 36 * 8 + 16400
    # a refused shape: the workgroup count is 0 (a count, never negative), the byte queries fail; both leave the text
    for fn, who, no in ((L.pk_activation_stats_blocks, "pk_activation_stats_blocks", 0), (L.pk_activation_stats_ws_bytes, "pk_activation_stats_ws_bytes", -1),
                        (L.pk_activation_quantiles_ws_bytes, "pk_activation_quantiles_ws_bytes", -1)):
        assert fn(2 ** 38 // 8 + 1, 8) == no and err() == f"{who}: M={2 ** 38 // 8 + 1} rows of C=8: M C outside [1, 2^38]"
        assert fn(2 ** 62, 8) == no and fn(0, 8) == no and fn(-1, 8) == no
        assert fn(10, 12) == no and err() == f"{who}: C=12 must be a multiple of 8 (16-byte bf16 chunks)"
    assert L.pk_activation_stats_slab(2056) == -1 and L.pk_activation_stats_slab(4) == -1
    # the largest workspace fits the int the queries return
    assert 0 < L.pk_activation_stats_ws_bytes(2 ** 38 // 2048, 2048) == 512 * (36 * 2048 + 16400) < 2 ** 31


# ------------------------------------------------------------------------------------------------ the restatement itself
def _few_hundred(seed=0, M=37, C=16):
    g = np.random.default_rng(seed)
    v = (g.standard_normal((M, C)) * np.exp2(g.integers(-20, 21, (M, C)))).astype(np.float32)
    bits = anp.from_f32(v)
    bits[0, :6] = [0x0000, 0x8000, 0x7f80, 0xff80, 0x7fc1, 0x0001]       # +0, -0, +inf, -inf, NaN, the smallest subnormal
    bits[1, :4] = [0x7f7f, 0xff7f, 0x8001, 0x007f]                       # +-max finite, the negative subnormals' ends
    bits[:, 7] = 0
    return bits


def test_restatement_against_plain_numpy_on_a_few_hundred_values():
    bits = _few_hundred()
    M, C = bits.shape
    for c_used in (C, C - 3, 1):
        rec, hist = anp.stats(bits, c_used)
        f = anp.to_f32(bits)[:, :c_used].astype(np.float64)
        fin = np.isfinite(f)
        assert rec["n"].tolist() == [M] * c_used and np.array_equal(rec["n_nonfinite"], (~fin).sum(0))
        assert np.array_equal(rec["n_zero"], ((f == 0) & fin).sum(0)) and np.array_equal(rec["n_negative"], ((f < 0) & fin).sum(0))
        for j in range(c_used):
            col = f[fin[:, j], j]
            assert abs(rec["sum"][j] - math.fsum(col)) <= len(col) * 2.0 ** -53 * np.abs(col).sum()
            assert abs(rec["sumsq"][j] - math.fsum(col * col)) <= len(col) * 2.0 ** -53 * (col * col).sum()
            assert rec["min"][j] == col.min() and rec["max"][j] == col.max()
            assert not np.signbit(rec["min"][j]) or rec["min"][j] < 0      # -0 is read as +0
        assert hist.sum() == fin.sum()
        want, _ = np.histogram(f[fin], bins=anp.bin_edges()[8:4089])       # the finite bins; numpy closes the last one, nothing lies on it
        assert np.array_equal(hist[8:4088], want) and not hist[:8].any() and not hist[4088:].any()
        q = [0.0, 0.25, 0.5, 0.75, 1.0, 0.123]
        order = anp.quantiles(bits, q, c_used)
        v = np.sort(f[fin])
        assert np.array_equal(order[:, 0].astype(np.float64) + 0.0, v[np.floor(np.array(q) * (len(v) - 1)).astype(int)] + 0.0)
        from infantposeestimation_gaussianbias_amd.utils import metrics
        got = metrics._quantile_values(order[None], np.array([len(v)]), np.array(q))[0]
        assert np.allclose(got, np.quantile(v, q), rtol=1e-15, atol=0)
    full = anp.stats(bits)[0]
    assert full["n_zero"][:2].tolist() == [1, 1] and full["n_nonfinite"][:6].tolist() == [0, 0, 1, 1, 1, 0] and full["n_zero"][7] == M
    assert full["n_negative"][1] == (anp.to_f32(bits[:, 1]) < 0).sum() and full["min"][7] == 0 and full["max"][7] == 0
    two = anp.accumulate(anp.stats(bits), anp.stats(bits[::-1]))
    assert np.array_equal(two[1], 2 * anp.stats(bits)[1]) and np.array_equal(two[0]["n"], [2 * M] * C)
    assert np.isnan(anp.quantiles(np.full((3, 8), 0x7fc0, np.uint16), [0.5])).all()


def test_ordered_sum_is_the_documented_order():
    """Three values whose fp64 sum depends on the order, one per workgroup-level of the documented order."""
    C = 8
    G, slab = 256, 1024
    big, one = 2.0 ** 53, 1.0
    # rows 0 and G belong to thread r = 0 (passes u = 0 and 1), row 1 to thread r = 1: (big + 1) + (-big) per thread order is
    # thread 0: big + (-big) = 0, then + thread 1's 1.0 = 1.0; ascending-row order would give (big + 1) - big = 0.0
    d = np.zeros((G + 1, C))
    d[0, 0], d[1, 0], d[G, 0] = big, one, -big
    assert anp._ordered_sum(d, G + 1, C)[0] == 1.0 and (big + one) - big == 0.0
    # workgroups: slab 0 -> workgroup 0, slab 1 -> workgroup 1; left to right over workgroups
    d = np.zeros((2 * slab + 1, C))
    d[0, 1], d[slab, 1], d[1, 1] = big, -big, one                 # workgroup 0: thread 0 big, thread 1 one -> big (+1 lost); + workgroup 1
    assert anp._ordered_sum(d, 2 * slab + 1, C)[1] == 0.0
    assert anp.split(2 * slab + 1, C) == (3, G, slab)


def test_every_bf16_pattern_lands_in_the_bin_whose_edges_contain_it():
    from infantposeestimation_gaussianbias_amd import hipops
    edges = anp.bin_edges()
    assert np.array_equal(edges, hipops.activation_bin_edges()) and len(edges) == 4097
    assert np.all(edges[9:4089] > edges[8:4088]) and np.all(edges[1:] >= edges[:-1])
    assert edges[2048] == 0.0 and not np.signbit(edges[2048]) and np.isneginf(edges[:8]).all() and np.isposinf(edges[4088:]).all()
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    b = anp.bin_of(bits).astype(np.int64)
    fin = ~anp.is_nonfinite(bits)
    with np.errstate(invalid="ignore"):                           # signalling NaN patterns widen with a flag
        f = anp.to_f32(bits).astype(np.float64)
    assert fin.sum() == 65536 - 2 * 128 and np.array_equal(fin, np.isfinite(f))
    assert np.all(edges[b[fin]] <= f[fin]) and np.all(f[fin] < edges[b[fin] + 1])
    assert b[fin].min() == 8 and b[fin].max() == 4087 and b[0x0000] == b[0x8000] == anp.ZERO_BIN
    assert set(b[~fin]) <= set(range(0, 8)) | set(range(4088, 4096))
    # every edge of a finite bin is an exact bf16 value, and the key orders the values
    assert np.array_equal(anp.to_f32(anp.from_f32(edges[8:4089].astype(np.float32))).astype(np.float64), edges[8:4089])
    order = np.argsort(anp.key_of(bits[fin]), kind="stable")
    assert np.all(np.diff(f[fin][order]) >= 0)
    assert np.array_equal(anp.value_of_key(anp.key_of(bits[fin & (bits != 0x8000)])).view(np.uint32) >> 16, bits[fin & (bits != 0x8000)])


# ------------------------------------------------------------------------------------------------ op layer and utils
def test_op_layer_checks_shapes_and_has_no_host_path(monkeypatch):
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(hipops, "call", no_launch)
    with pytest.raises(PoseKernelError):
        hipops.activation_stats(torch.zeros(4, 8, dtype=torch.bfloat16))
    with pytest.raises(PoseKernelError):
        hipops.activation_quantiles(torch.zeros(4, 8, dtype=torch.bfloat16), torch.zeros(4096, dtype=torch.int64), [0.5])
    assert hipops.activation_stats_blocks(1, 8) == (1, 1024)


def test_activation_report_refuses_a_cpu_tensor_and_a_model_in_training_mode():
    from infantposeestimation_gaussianbias_amd import utils
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    assert {"activation_report", "ActivationAnalyzer", "ActivationCollector"} <= set(utils.__all__)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3))
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        utils.activation_report(model, torch.zeros(1, 3, 16, 16))
    model.eval()
    with pytest.raises(PoseKernelError):
        utils.activation_report(model, torch.zeros(1, 3, 16, 16))
    with pytest.raises(PoseKernelError):
        utils.ActivationAnalyzer.analyze_activation_distribution(torch.zeros(1, 8, 4, 4))
    for bad in (dict(quantiles=[1.5]), dict(quantiles=[0.1] * 17), dict(max_batches=0)):
        with pytest.raises(ValueError):
            utils.activation_report(model, torch.zeros(1, 3, 16, 16), **bad)


def test_validate_parser_accepts_the_two_flags():
    import validate as V
    p = V.build_parser()
    args = p.parse_args(["--checkpoint", "x.pth"])
    assert args.activation_report is None and args.activation_batches == 1
    args = p.parse_args(["--checkpoint", "x.pth", "--activation_report", "act.json", "--activation_batches", "3"])
    assert args.activation_report == "act.json" and args.activation_batches == 3
