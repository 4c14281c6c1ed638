"""Host trace (tests/op_trace.py's recorder, no device) of nnops.conv_bn_act_out: a head branch Conv2d(16, C, 3) + BatchNorm + ReLU +
Conv2d(C, N, 1) with the row threshold lowered takes pk_conv2d_nhwc, pk_bn_finalize, pk_bn_out1x1_fwd and, in backward, the converter, the
output conv's weight gradient exactly as head_out launches it, the composed pk_bn_out1x1_bwd and the 3x3 conv's data and weight gradient;
the output conv's data gradient has no buffer: the only buffers of its size are raw, the activated tensor and draw.  With the route switched
off, or below its threshold, the module takes today's conv_bn_act + head_out calls; the cases of the recorded fixture stay line for line as
recorded with the threshold lowered."""
import functools
import lzma
import os

import pytest

import op_trace

B, H, W, CIN = 2, 6, 5, 16
M = B * H * W
FORMS = ((256, 17, False), (256, 34, False), (128, 17, True))
ENV = ("PK_BN_OUT1X1", "PK_BN_OUT1X1_MIN_ROWS", "PK_BN_OUT1X1_MAX_GRID")
FWD = ["pk_conv2d_nhwc", "pk_bn_finalize", "pk_bn_out1x1_fwd"]
BWD = ["pk_nchw_f32_to_nhwc_bf16", "pk_wgrad_bf16", "pk_bn_out1x1_bwd", "pk_conv2d_nhwc", "pk_wgrad_bf16"]
STORED = ["pk_conv2d_nhwc", "pk_bn_train_fwd", "pk_conv2d_nhwc", "pk_nchw_f32_to_nhwc_bf16", "pk_conv2d_nhwc", "pk_wgrad_bf16", "pk_bn_bwd",
          "pk_conv2d_nhwc", "pk_wgrad_bf16"]


def _build(C, N, softplus, cin=CIN):
    def build():
        m = op_trace.nn.Sequential(*op_trace.conv_bn(cin, C, 3), op_trace.nn.Conv2d(C, N, 1))
        return m, dict(x=op_trace.fmap(B, H, W, cin)), lambda m, i, drop: op_trace.nnops.conv_bn_act_out(i["x"], m[0], m[1], m[2], softplus, True)
    return build


def _trace(mp, regime, build, grad=True, **env):
    for k in ENV:
        mp.delenv(k, raising=False)
    mp.setitem(op_trace.CASES, "bn_out1x1", (build, dict(grad=grad, env=env)))
    return op_trace.trace("bn_out1x1", regime, mp)


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
    return out


def _rows(lines, start, stop):
    """the `row` lines between the markers `start` and `stop` as dicts"""
    i, j = lines.index(start), lines.index(stop)
    return [dict(f.split("=", 1) for f in ln.split()[1:]) for ln in lines[i + 1:j] if ln.startswith("  row ")]


def _stored(mp, regime, C, N, softplus):
    return _trace(mp, regime, _build(C, N, softplus), PK_BN_OUT1X1_MIN_ROWS="1", PK_BN_OUT1X1="0")


@pytest.mark.parametrize("C,N,softplus", FORMS)
@pytest.mark.parametrize("regime", op_trace.REGIMES)
def test_fused_route_call_sequence(regime, C, N, softplus, monkeypatch):
    lines = _trace(monkeypatch, regime, _build(C, N, softplus), PK_BN_OUT1X1_MIN_ROWS="1")
    calls = _calls(lines)
    names = [n for n, _ in calls if n not in ("pk_pack_weights", "pk_reduce_many")]
    assert names == FWD + BWD, names
    assert not {"pk_bn_train_fwd", "pk_bn_bwd", "pk_bn_act"} & set(names)
    arg = {}
    for n, a in calls:
        arg.setdefault(n, a)
    conv, fin, fw, cv, bw = arg["pk_conv2d_nhwc"], arg["pk_bn_finalize"], arg["pk_bn_out1x1_fwd"], arg["pk_nchw_f32_to_nhwc_bf16"], arg["pk_bn_out1x1_bwd"]
    x, raw, part = conv[0], conv[2], conv[3]
    assert fin[0] == part and fin[1:4] == [str((M + 127) // 128), str(C), str(M)]
    scale, shift, mean, rstd = fin[11:15]
    assert fw[:3] == [raw, scale, shift] and fw[8:] == [str(M), str(C), str(N), str(H * W), "1" if softplus else "0", "null"]
    t, out, mask = fw[5], fw[6], fw[7]
    # converter: dout (and the maps, for softplus) -> g with up8(N) channels, as head_out asks for it
    Np = -(-N // 8) * 8
    assert cv[1] == (out if softplus else "null") and cv[3:8] == [str(B), str(N), str(H), str(W), str(Np)]
    g = cv[2]
    # the output conv's weight gradient reads the saved t and g; BatchNorm backward the SAME raw / mask / statistics as forward and g
    wg1 = arg["pk_wgrad_bf16"]
    assert wg1[:2] == [t, g] and wg1[10:15] == [str(M), str(Np), str(C), "1", "1"]
    assert bw[:3] == [g, raw, mask] and bw[4:7] == [mean, rstd, fin[4]] and bw[12:15] == [str(M), str(C), str(N)]
    draw = bw[11]
    dgrad = [a for n, a in calls if n == "pk_conv2d_nhwc"][1]
    wg3 = [a for n, a in calls if n == "pk_wgrad_bf16"][1]
    assert dgrad[0] == draw and wg3[0] == x and wg3[1] == draw
    # no buffer for the output conv's data gradient: the buffers of its size are raw, t and draw (dx is 16 channels wide here)
    size = M * C * 2
    bufs = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("buffer ")}
    big = sorted(b for b, n in bufs.items() if n == size)
    assert big == sorted(p.split("+")[0] for p in (raw, t, draw)), (big, raw, t, draw)
    # the stored route has one more (the data gradient), and the same reductions, sinks and returned gradients for the output conv
    want = _stored(monkeypatch, regime, C, N, softplus)
    wbufs = [int(ln.split()[2]) for ln in want if ln.startswith("buffer ")]
    assert sum(1 for n in wbufs if n == size) == 4
    for kind in ("pending", "param"):
        rows = lambda ls: sorted((ln.split("part=")[0] + " ".join(f for f in ln.split() if f.split("=")[0] in ("stride", "S", "K", "layout", "N", "T", "Cin")))  # noqa: E731
                                 if ln.startswith("  row") else ln for ln in ls if ln.startswith(("  row", "param ")))
        assert rows(lines[lines.index("pending"):]) == rows(want[want.index("pending"):]), kind
    ret = [ln for ln in lines if ln.startswith("return _ConvBnActOut")]
    assert len(ret) == 1 and f"bfloat16[{B}, {H}, {W}, {CIN}]" in ret[0]
    if regime == "a":                              # no sinks: autograd receives every gradient, the output conv's in its parameters' shapes
        assert f"float32[{N}, {C}, 1, 1]" in ret[0] and f"float32[{N}]" in ret[0]


@pytest.mark.parametrize("env", [dict(PK_BN_OUT1X1_MIN_ROWS="1", PK_BN_OUT1X1="0"), {}])
def test_route_off_takes_todays_calls(env, monkeypatch):
    """switched off; and 60 rows are below the default threshold"""
    for regime in op_trace.REGIMES:
        names = [n for n, _ in _calls(_trace(monkeypatch, regime, _build(256, 17, False), **env)) if n not in ("pk_pack_weights", "pk_reduce_many")]
        assert names == STORED, (regime, names)


def test_no_grad_and_observer_take_todays_calls(monkeypatch):
    """no autograd recording, or an activation collector installed (its taps need the activated tensor): conv_bn_act + head_out"""
    names = [n for n, _ in _calls(_trace(monkeypatch, "a", _build(256, 17, False), grad=False, PK_BN_OUT1X1_MIN_ROWS="1")) if n != "pk_pack_weights"]
    assert names == ["pk_conv2d_nhwc", "pk_bn_train_fwd", "pk_conv2d_nhwc"], names

    class Collector:
        def tap(self, *a):
            pass

    with op_trace.nnops.observe(Collector()):
        names = [n for n, _ in _calls(_trace(monkeypatch, "b", _build(256, 17, False), PK_BN_OUT1X1_MIN_ROWS="1")) if n not in ("pk_pack_weights", "pk_reduce_many")]
    assert names == STORED, names


def test_unsupported_widths_take_todays_calls(monkeypatch):
    """a hidden width the library is not built for (64) stays on the stored route even with the threshold lowered"""
    assert op_trace._lib.lib.pk_bn_out1x1_supported(M, 64, 17) == 0
    names = [n for n, _ in _calls(_trace(monkeypatch, "b", _build(64, 17, False), PK_BN_OUT1X1_MIN_ROWS="1")) if n not in ("pk_pack_weights", "pk_reduce_many")]
    assert names == STORED, names


def test_supported_rule(monkeypatch):
    L = op_trace._lib.lib
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    assert L.pk_bn_out1x1_supported(196608, 256, 17) == 1 and L.pk_bn_out1x1_supported(196608, 256, 34) == 1 and L.pk_bn_out1x1_supported(196608, 128, 17) == 1
    assert L.pk_bn_out1x1_supported(32768, 256, 17) == 1 and L.pk_bn_out1x1_supported(32767, 256, 17) == 0
    assert L.pk_bn_out1x1_supported(196608, 256, 49) == 0 and L.pk_bn_out1x1_supported(196608, 512, 17) == 0
    monkeypatch.setenv("PK_BN_OUT1X1", "0")
    assert L.pk_bn_out1x1_supported(196608, 256, 17) == 0


@pytest.mark.parametrize("name", [n for n in op_trace.CASES if n.startswith(("conv", "stem", "residual", "deconv", "head_out", "exchange"))])
def test_recorded_cases_are_untouched_with_the_threshold_lowered(name, monkeypatch):
    want = _recorded()
    monkeypatch.setenv("PK_BN_OUT1X1_MIN_ROWS", "1")
    for regime in op_trace.REGIMES:
        assert op_trace.trace(name, regime, monkeypatch) == want[f"{name}/{regime}"], f"{name}/{regime}"
