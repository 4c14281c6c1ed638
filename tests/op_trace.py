"""Host trace of the op layer (nnops.py, exchange.py): what every autograd Function launches, queues and hands to autograd.

Every launch of the op layer goes through `_lib.call` and `_lib.stream_ptr`, imported by name into nnops, exchange and hipops.  Here
`call` is replaced by a recorder and `stream_ptr` by a constant, so the Functions run forward and backward on CPU bf16 tensors without
a device: nothing executes, the size queries (host functions of the real library) answer as usual.  Per case and gradient regime the
trace holds, in order

    call    the C-ABI entry and its arguments: scalars verbatim, pointers as null or b<buffer id>+<byte offset> (ids by first appearance;
            parameters, sinks, buffers and inputs are registered up front), descriptor tables decoded field by field
    return  per position of a backward's result: None, or dtype and shape of the tensor autograd received
    pending the rows left in nnops._PENDING after backward, then what finalize_deferred() launches
    param   per parameter: sink_written, _pk_used;   ws: tag and element count of every workspace on its sink
    buffer  size and name of every buffer the trace refers to

tests/test_op_trace_host.py compares this with tests/golden/op_trace.txt.xz section by section.  The fixture was recorded from the
commit before the gradient-destination / slab-reduction paths of nnops.py were unified, with this recorder as it stands:

    python tests/op_trace.py | xz -9e > tests/golden/op_trace.txt.xz

Regimes: a = no gradient sinks; b = every parameter has one (DropPath scales present); c = as b with POSE_DEFER_REDUCE=0, no scales;
d = only the conv / linear weight matrices have one (biases, norm parameters, the rel-pos table do not).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from infantposeestimation_gaussianbias_amd import _lib, exchange as xg, hipops, nnops  # noqa: E402
from infantposeestimation_gaussianbias_amd.models._blocks import make_fuse_layers  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
REGIMES = ("a", "b", "c", "d")
GROUP_DT = {"pk_conv2d_group": xg.CONV_DT, "pk_bn_train_fwd_group": xg.BNF_DT, "pk_bn_bwd_group": xg.BNB_DT,
            "pk_fuse_sum_group": xg.FUSE_DT, "pk_upsample_bwd_group": xg.UPB_DT, "pk_wgrad_group": xg.WG_DT}
SYMBOLS = _lib.declared_symbols()


class Recorder:
    def __init__(self):
        self.lines = []
        self.spans = []          # [start, end, id or None, label, storage]: every storage seen, kept alive so no address is reused
        self.sinks = []
        self.n_ids = 0

    # ---- buffers
    def note(self, t, label=""):
        st = t.untyped_storage()
        p = st.data_ptr()
        if p and not any(s[0] == p for s in self.spans):
            self.spans.append([p, p + st.nbytes(), None, label, st])
        return t

    def ref(self, ptr):
        if not ptr:
            return "null"
        for sk in self.sinks:                      # workspaces are allocated inside the op layer, on the sink they serve
            for tag, ws in getattr(sk, "_pk_ws", {}).items():
                self.note(ws, f"ws:{tag}")
        for s in self.spans:
            if s[0] <= ptr < s[1]:
                if s[2] is None:
                    s[2], self.n_ids = self.n_ids, self.n_ids + 1
                return f"b{s[2]}+{ptr - s[0]}"
        raise AssertionError(f"pointer {ptr:#x} lies in no known buffer")

    # ---- descriptor tables
    def rows(self, arr, pointers):
        out = []
        for r in arr:
            f = []
            for k in arr.dtype.names:
                v = r[k]
                if np.ndim(v):
                    f.append(f"{k}=[" + ",".join(self.ref(int(e)) if k in pointers else str(e.item()) for e in v) + "]")
                else:
                    f.append(f"{k}={self.ref(int(v)) if k in pointers else v.item()}")
            out.append("  row " + " ".join(f))
        return out

    def reduce_rows(self, rows):
        return self.rows(np.array([tuple(r) for r in rows], dtype=nnops._REDUCE_DTYPE), ("part", "out"))

    @staticmethod
    def host(ptr, n, ctype):
        return list((ctype * n).from_address(ptr))

    # ---- the two chokepoints
    def call(self, name, *args):
        _lib.CALLS[0] += 1
        kinds = SYMBOLS[name][1]
        assert len(kinds) == len(args), f"{name}: {len(args)} arguments for {len(kinds)} parameters"
        args, extra = list(args), []
        if name in GROUP_DT:
            dt = GROUP_DT[name]
            arr = np.frombuffer((ctypes.c_char * (dt.itemsize * args[1])).from_address(args[0]), dtype=dt)
            extra, args[0] = self.rows(arr, [k for k in dt.names if dt[k].base == np.dtype("<u8")]), "<desc>"
        elif name == "pk_reduce_many":
            extra = self.rows(args[0].numpy().view(nnops._REDUCE_DTYPE), ("part", "out"))
            args[:3] = ["<desc>", str(args[1].tolist()), str(args[2].tolist())]
        elif name == "pk_pack_weights":
            extra = self.rows(args[1].numpy().view(nnops._PACK_DTYPE), ("src",))
            args[1:4] = ["<desc>", str(args[2].tolist()), str(args[3].tolist())]
        elif name == "pk_fuse_sum":
            n = args[3]
            args[:3] = ["[" + ",".join(self.ref(p) for p in self.host(args[0], n, ctypes.c_int64)) + "]",
                        str(self.host(args[1], n, ctypes.c_int32)), str(self.host(args[2], n, ctypes.c_int32))]
        out = []
        for a, kind in zip(args, kinds):
            if isinstance(a, str):
                out.append(a)
            elif a is None:
                out.append("null")
            elif hasattr(a, "data_ptr"):
                out.append(self.ref(self.note(a).data_ptr()))
            elif kind is ctypes.c_void_p:
                out.append(self.ref(a))
            else:
                out.append(repr(a))
        self.lines.append(f"call {name}(" + ", ".join(out) + ")")
        self.lines += extra

    def returned(self, cls, res):
        res = res if isinstance(res, tuple) else (res,)
        self.lines.append(f"return {cls.__name__}: " + ", ".join(
            "None" if r is None else f"{str(r.dtype)[6:]}{list(r.shape)}" for r in res))


class _FakeCuda:
    is_current_stream_capturing = staticmethod(lambda: False)
    current_device = staticmethod(lambda: 0)
    current_stream = staticmethod(lambda: None)


class _HostTorch:
    """`torch` as nnops sees it here: no device, so tables meant for the GPU stay on the CPU."""
    cuda = _FakeCuda

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def device(*a):
        return torch.device("cpu")


class _RowsByMapHost(torch.autograd.Function):
    """hipops._RowsByMap without its is_cuda check (the only op of the deconv stack that lives outside nnops)."""

    @staticmethod
    def forward(ctx, x2d, rowmap, n_out, scatter):
        x2d = x2d.contiguous()
        out = torch.empty((n_out, x2d.shape[1]), dtype=x2d.dtype)
        hipops.call("pk_rows_by_map", x2d, out, rowmap, rowmap.numel(), x2d.shape[1] * x2d.element_size(), 1 if scatter else 0,
                    hipops.stream_ptr())
        ctx.save_for_backward(rowmap)
        ctx.meta = (x2d.shape[0], scatter)
        return out

    @staticmethod
    def backward(ctx, g):
        return _RowsByMapHost.apply(g, ctx.saved_tensors[0], ctx.meta[0], not ctx.meta[1]), None, None, None


def functions():
    fs = [v for v in vars(nnops).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == nnops.__name__]
    return fs + [xg._Unit]


def install(mp, rec):
    """Patch the op layer's chokepoints through the pytest MonkeyPatch `mp`."""
    for mod in (nnops, xg, hipops):
        mp.setattr(mod, "call", rec.call)
        mp.setattr(mod, "stream_ptr", lambda: 0)
    mp.setattr(nnops, "torch", _HostTorch())
    mp.setattr(torch.Tensor, "record_stream", lambda self, s: None)
    mp.setattr(hipops, "rows_by_map", _RowsByMapHost.apply)
    alloc = nnops._e
    mp.setattr(nnops, "_e", lambda *a: rec.note(alloc(*a)))
    for cls in functions():
        def backward(ctx, *g, _cls=cls, _orig=cls.backward):
            res = _orig(ctx, *g)
            rec.returned(_cls, res)
            return res
        mp.setattr(cls, "backward", staticmethod(backward))
    for cache in (nnops._TABLES, nnops._MAPS, nnops._SHUFFLE_MAPS, nnops._ZERO_TABLES):
        cache.clear()
    del nnops._PENDING[:]


# ================================================================================================ cases
def conv_bn(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride, k // 2, bias=False), nn.BatchNorm2d(cout)


def fmap(B, H, W, C, grad=True):
    return torch.zeros(B, H, W, C, dtype=BF16, requires_grad=grad)


class Block(nn.Module):
    """The attribute names nnops.window_block reads from an HRFormer block."""

    def __init__(self, C, heads, rpe=True):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(C), nn.LayerNorm(C)
        self.attn, self.mlp = nn.Module(), nn.Module()
        self.attn.qkv, self.attn.proj, self.attn.num_heads = nn.Linear(C, 3 * C), nn.Linear(C, C), heads
        if rpe:
            self.attn.relative_position_bias_table = nn.Parameter(torch.zeros(169, heads))
        self.mlp.fc1, self.mlp.fc2 = nn.Linear(C, 4 * C), nn.Linear(4 * C, C)

    def attn_args(self, heads):
        a = self.attn
        return (self.norm1.weight, self.norm1.bias, nnops.rel_table(a, heads), a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias)

    def mlp_args(self):
        m = self.mlp
        return (self.norm2.weight, self.norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)


CASES = {}      # name -> (build, options); build() -> (model, inputs {name: tensor}, run(model, inputs, drop) -> output(s))


def case(name, grad=True, env=None):
    def deco(build):
        CASES[name] = (build, dict(grad=grad, env=env or {}))
        return build
    return deco


def _conv_case(name, k, stride, relu, residual=False, training=True, grad=True):
    @case(name, grad=grad)
    def build():
        m = nn.Sequential(*conv_bn(16, 24, k, stride))
        B, Hs, Ws, Cin, Ho, Wo = nnops._conv_geometry(torch.empty(2, 6, 5, 16), k, stride)
        ins = dict(x=fmap(2, 6, 5, 16, grad))
        if residual:
            ins["res"] = fmap(2, Ho, Wo, 24, grad)
        return m, ins, lambda m, i, drop: nnops.conv_bn_act(i["x"], m[0], m[1], relu, i.get("res"), training)


_conv_case("conv3x3_s1_relu_train", 3, 1, True)
_conv_case("conv3x3_s2_train", 3, 2, False)
_conv_case("conv1x1_s1_relu_res_train", 1, 1, True, residual=True)
_conv_case("conv1x1_s2_train", 1, 2, False)
_conv_case("conv3x3_s1_res_train", 3, 1, False, residual=True)
_conv_case("conv3x3_s1_relu_res_eval_grad", 3, 1, True, residual=True, training=False)
_conv_case("conv1x1_s1_eval_grad", 1, 1, False, training=False)
_conv_case("conv3x3_s1_relu_res_infer", 3, 1, True, residual=True, training=False, grad=False)
_conv_case("conv3x3_s2_train_no_grad", 3, 2, True, grad=False)


@case("stem_3_of_8_channels")
def _stem():
    m = nn.Sequential(*conv_bn(3, 16, 3, 2))
    return m, dict(x=fmap(2, 6, 5, 8, False)), lambda m, i, drop: nnops.conv_bn_act(i["x"], m[0], m[1], True, None, True)


def _residual(training):
    def build():
        m = nn.Sequential(*conv_bn(16, 16, 3), *conv_bn(16, 16, 3), *conv_bn(16, 16, 3))
        return m, dict(x=fmap(2, 6, 5, 16)), lambda m, i, drop: nnops.residual_block(i["x"], (m[0], m[1]), [(m[2], m[3])], (m[4], m[5]), training)
    return build


case("residual_block_train")(_residual(True))
case("residual_block_eval_grad")(_residual(False))


def _deconv(k):
    @case(f"deconv_k{k}")
    def build():
        m = nn.Sequential(nn.ConvTranspose2d(16, 24, k, 2, (k - 1) // 2, bias=False), nn.BatchNorm2d(24))
        return m, dict(x=fmap(2, 6, 5, 16)), lambda m, i, drop: nnops.deconv_bn_relu(i["x"], m[0], m[1], True)


_deconv(2)
_deconv(4)


def _head(softplus):
    @case("head_out_softplus" if softplus else "head_out")
    def build():
        m = nn.Sequential(nn.Conv2d(16, 17, 1))
        return m, dict(x=fmap(2, 6, 5, 16)), lambda m, i, drop: nnops.head_out(i["x"], m[0], softplus)


_head(False)
_head(True)


def _half(name, fn, C, heads, rpe=True, attn=True, extra=()):
    @case(name)
    def build():
        blk = Block(C, heads, rpe)

        def run(m, i, drop):
            args = m.attn_args(heads) if attn else m.mlp_args()
            return fn.apply(i["x"], *args, drop, *((heads,) if attn else ()), *extra)
        return blk, dict(x=fmap(2, 9, 10, C)), run


_half("attn_half_c32", nnops._AttnHalf, 32, 1)
_half("attn_half_c64_2heads", nnops._AttnHalf, 64, 2)
_half("attn_half_c_real_attn_scale", nnops._AttnHalf, 32, 1, extra=(24, 0.2))
_half("attn_half_zero_table", nnops._AttnHalf, 32, 1, rpe=False)
_half("attn_half_fused", nnops._AttnHalfFused, 32, 1)
_half("attn_half_fused_zero_table", nnops._AttnHalfFused, 32, 1, rpe=False)
_half("attn_half_fused_c64_2heads", nnops._AttnHalfFused, 64, 2)
_half("mlp_half_c32", nnops._MlpHalf, 32, 1, attn=False)
_half("mlp_half_c_real", nnops._MlpHalf, 32, 1, attn=False, extra=(24,))
_half("mlp_half_fused_c32", nnops._MlpHalfFused, 32, 1, attn=False)
_half("mlp_half_fused_c64", nnops._MlpHalfFused, 64, 2, attn=False)


def _window_block(name, C, heads, grad=True, rpe=True):
    @case(name, grad=grad)
    def build():
        return Block(C, heads, rpe), dict(x=fmap(2, 9, 10, C, grad)), lambda m, i, drop: nnops.window_block(i["x"], m, heads, drop, drop)


_window_block("window_block_c32", 32, 1)
_window_block("window_block_c64", 64, 2)
_window_block("window_block_c32_zero_table", 32, 1, rpe=False)
_window_block("window_block_c32_no_grad", 32, 1, grad=False)
_window_block("window_block_c64_no_grad", 64, 2, grad=False)
_window_block("window_block_c80_no_grad", 80, 2, grad=False)


@case("window_attention_tokens")
def _tokens():
    return (Block(32, 1), dict(tok=torch.zeros(4 * 49, 32, dtype=BF16, requires_grad=True)),
            lambda m, i, drop: nnops.window_attention_tokens(i["tok"], m.attn, 1))


@case("mlp_rows")
def _rows():
    return Block(32, 1), dict(x=torch.zeros(45, 32, dtype=BF16, requires_grad=True)), lambda m, i, drop: nnops.mlp_rows(i["x"], m.mlp)


def _fuse_sum(relu):
    @case("fuse_sum_relu" if relu else "fuse_sum")
    def build():
        ins = dict(x0=fmap(2, 12, 10, 16), x1=fmap(2, 6, 5, 16), x2=fmap(2, 3, 3, 16), x3=fmap(2, 12, 10, 16))
        return nn.Module(), ins, lambda m, i, drop: nnops.fuse_sum(list(i.values()), relu)


_fuse_sum(True)
_fuse_sum(False)


@case("sum_same_shape", grad=False)
def _sum():
    ins = dict(x0=fmap(2, 6, 5, 16, False), x1=fmap(2, 6, 5, 16, False), x2=fmap(2, 6, 5, 16, False))
    return nn.Module(), ins, lambda m, i, drop: nnops.sum_same_shape(list(i.values()))


def _exchange(n, mode):
    """mode: "unit" = nnops.exchange as one grouped unit; "grouped" / "layers" = nnops.exchange_output per output, grouped launches or
    one conv_bn_act per layer."""
    @case(f"exchange_{n}_{mode}", env={"POSE_GROUPED_EXCHANGE": {"unit": "2", "grouped": "1", "layers": "0"}[mode]})
    def build():
        fuse = make_fuse_layers([16, 32, 64][:n])
        ins = {f"x{j}": fmap(2, 12 >> j, (10, 5, 3)[j], 16 << j) for j in range(n)}

        def run(m, i, drop):
            xs = list(i.values())
            if mode == "unit":
                return nnops.exchange(xs, m, True)
            return [nnops.exchange_output(o, xs, m, True) for o in range(n)]
        return fuse, ins, run


for _n in (2, 3):
    for _mode in ("unit", "grouped", "layers"):
        _exchange(_n, _mode)


# ================================================================================================ driver
def is_matrix(name, p):
    return p.dim() >= 2 and "relative_position_bias_table" not in name


def trace(name, regime, mp):
    """-> the trace of one case under one regime, a list of lines."""
    build, opt = CASES[name]
    rec = Recorder()
    install(mp, rec)
    mp.setenv("POSE_DEFER_REDUCE", "0" if regime == "c" else "1")
    for k, v in opt["env"].items():
        mp.setenv(k, v)
    model, ins, run = build()
    params = dict(model.named_parameters())
    for k, p in params.items():
        rec.note(p, f"param:{k}")
        if regime in "bc" or (regime == "d" and is_matrix(k, p)):
            p._pk_grad_sink = rec.note(torch.empty(p.shape, dtype=F32), f"sink:{k}")
            rec.sinks.append(p._pk_grad_sink)
    for k, b in model.named_buffers():
        rec.note(b, f"buffer:{k}")
    for k, t in ins.items():
        rec.note(t, f"in:{k}")
    drop = rec.note(torch.ones(2), "in:drop") if regime == "b" else None
    nnops.begin_grad_epoch()
    with torch.enable_grad() if opt["grad"] else torch.no_grad(), nnops.use_weights(model):
        out = run(model, ins, drop)
        out = [out] if torch.is_tensor(out) else list(out)
        if opt["grad"]:
            rec.lines.append("backward")
            torch.autograd.backward(out, [rec.note(torch.zeros_like(o), f"in:dy{q}") for q, o in enumerate(out)])
    rec.lines += ["pending"] + rec.reduce_rows(nnops._PENDING) + ["finalize"]
    nnops.finalize_deferred()
    assert not nnops._PENDING
    for k, p in params.items():
        ws = getattr(getattr(p, "_pk_grad_sink", None), "_pk_ws", {})
        rec.lines.append(f"param {k}: sink_written={nnops.sink_written(p)} used={getattr(p, '_pk_used', False)} ws=" +
                         ",".join(f"{t}:{w.numel()}" for t, w in ws.items()))
    rec.lines += [f"buffer b{s[2]} {s[1] - s[0]} {s[3]}" for s in sorted((s for s in rec.spans if s[2] is not None), key=lambda s: s[2])]
    return rec.lines


def sections(text):
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            cur = out[line[3:]] = []
        else:
            cur.append(line)
    return out


if __name__ == "__main__":
    for _name in CASES:
        for _regime in REGIMES:
            with pytest.MonkeyPatch.context() as _mp:
                print(f"== {_name}/{_regime}")
                print("\n".join(trace(_name, _regime, _mp)))
