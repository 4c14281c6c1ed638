"""Host trace (tests/op_trace.py's recorder, no device) of the recomputing route of nnops.conv_bn_act: Conv2d(64, 256, 1) + BatchNorm
+ residual + ReLU with the row threshold lowered takes the statistics pass, pk_bn_finalize, the apply pass and, in backward, the composed
pk_conv1x1_bn_bwd in place of pk_conv2d_nhwc + pk_bn_train_fwd / pk_bn_bwd; the cases of the recorded fixture (16 -> 24, 16 -> 16 channels
and the rest) stay line for line as recorded with the threshold lowered, and the same module with the route switched off takes the
stored-raw calls."""
import functools
import lzma
import os

import pytest

import op_trace

B, H, W, CIN, COUT = 2, 16, 12, 64, 256
M = B * H * W


def _build():
    m = op_trace.nn.Sequential(*op_trace.conv_bn(CIN, COUT, 1))
    ins = dict(x=op_trace.fmap(B, H, W, CIN), res=op_trace.fmap(B, H, W, COUT))
    return m, ins, lambda m, i, drop: op_trace.nnops.conv_bn_act(i["x"], m[0], m[1], True, i["res"], True)


def _trace(mp, regime, **env):
    for k in ("PK_CONV1X1_BN", "PK_CONV1X1_BN_MIN_ROWS", "PK_CONV1X1_BN_MAX_GRID"):
        mp.delenv(k, raising=False)
    mp.setitem(op_trace.CASES, "conv1x1_64_256", (_build, dict(grad=True, env=env)))
    return op_trace.trace("conv1x1_64_256", regime, mp)


@functools.lru_cache(maxsize=None)
def _recorded():
    with lzma.open(os.path.join(op_trace.ROOT, "tests", "golden", "op_trace.txt.xz"), "rt") as f:
        return op_trace.sections(f.read())


def _calls(lines):
    out = []
    for ln in lines:
        if ln.startswith("call "):
            name, args = ln[5:].split("(", 1)
            out.append((name, [a.strip() for a in args.rstrip(")").split(",")]))
        elif not ln.startswith(" "):
            out.append((ln.split()[0].rstrip(":"), None))
    return out


@pytest.mark.parametrize("regime", op_trace.REGIMES)
def test_recomputing_route_call_sequence(regime, monkeypatch):
    lines = _trace(monkeypatch, regime, PK_CONV1X1_BN_MIN_ROWS="1")
    calls = _calls(lines)
    names = [n for n, a in calls if a is not None]
    bwd = names.index("pk_conv1x1_bn_bwd")
    assert names[:bwd] == ["pk_pack_weights", "pk_conv1x1_stats", "pk_bn_finalize", "pk_conv1x1_bn_act"] or \
        names[:bwd] == ["pk_conv1x1_stats", "pk_bn_finalize", "pk_conv1x1_bn_act"], names
    # everything after the BatchNorm backward is what the stored-raw route launches: data gradient, then the weight gradient
    assert names[bwd + 1:bwd + 3] == ["pk_conv2d_nhwc", "pk_wgrad_bf16"], names
    assert not {"pk_bn_train_fwd", "pk_bn_bwd", "pk_bn_act"} & set(names)
    assert names.count("pk_conv2d_nhwc") == 1
    arg = {n: a for n, a in calls if a is not None}
    st, fin, act, bw = arg["pk_conv1x1_stats"], arg["pk_bn_finalize"], arg["pk_conv1x1_bn_act"], arg["pk_conv1x1_bn_bwd"]
    x, wf, part = st[0], st[1], st[2]
    assert st[3:6] == [str(M), str(CIN), str(COUT)]
    assert fin[0] == part and fin[1:4] == [str((M + 127) // 128), str(COUT), str(M)]
    scale, shift, mean, rstd = fin[11:15]
    assert act[:4] == [x, wf, scale, shift] and act[4] != "null" and act[6] == "1" and act[7] != "null" and act[8:11] == [str(M), str(CIN), str(COUT)]
    y, mask = act[5], act[7]
    # backward: dy, the SAME x / packed weight / mask / statistics as forward, dresidual asked for; no buffer of y's size besides dy, draw, dres
    assert bw[1:5] == [x, wf, mean, rstd] and bw[11] != "null" and bw[12:16] == [str(M), str(CIN), str(COUT), "1"] and bw[16] == mask
    assert y not in bw
    draw = bw[10]
    assert arg["pk_conv2d_nhwc"][0] == draw and arg["pk_wgrad_bf16"][0] == x and arg["pk_wgrad_bf16"][1] == draw
    ret = [ln for ln in lines if ln.startswith("return _ConvBnAct")]
    assert len(ret) == 1 and f"bfloat16[{B}, {H}, {W}, {CIN}]" in ret[0] and f"bfloat16[{B}, {H}, {W}, {COUT}]" in ret[0]


def test_route_off_takes_the_stored_raw_calls(monkeypatch):
    for env in (dict(PK_CONV1X1_BN_MIN_ROWS="1", PK_CONV1X1_BN="0"), {}):        # switched off; 384 rows are below the default threshold
        names = [n for n, a in _calls(_trace(monkeypatch, "a", **env)) if a is not None]
        assert [n for n in names if n != "pk_pack_weights"] == ["pk_conv2d_nhwc", "pk_bn_train_fwd", "pk_bn_bwd", "pk_conv2d_nhwc", "pk_wgrad_bf16"], names


@pytest.mark.parametrize("name", [n for n in op_trace.CASES if n.startswith(("conv", "stem", "residual", "deconv", "head_out", "exchange"))])
def test_recorded_cases_are_untouched_with_the_threshold_lowered(name, monkeypatch):
    want = _recorded()
    monkeypatch.setenv("PK_CONV1X1_BN_MIN_ROWS", "1")
    for regime in op_trace.REGIMES:
        assert op_trace.trace(name, regime, monkeypatch) == want[f"{name}/{regime}"], f"{name}/{regime}"
