"""Further host-trace cases of the conv + BatchNorm family of nnops.py: what tests/golden/op_trace.txt.xz does not hold line for line.

    stem with an input gradient (pk_stem_dgrad, the weight gradient's slice / sink copy); the deconv stack in eval mode under autograd
    (_BnActOnly, the eval bit of pk_bn_bwd); the recomputing 1x1 route of conv_bn_act, alone in its forms and at the end of a bottleneck
    chain; a head branch through conv_bn_act_out, fused and on its stored fall-back; head_out with an 8-aligned output count.

CASES has the form of op_trace.CASES (name -> (build, options)) but is not part of it: tests/test_op_trace_conv_family_host.py places a
case into op_trace.CASES for the duration of one trace, so op_trace.txt.xz and its own test stay as they are.  Every case is B = 2 on a
6 x 5 map.  The fixture tests/golden/op_trace_conv.txt.xz was recorded from the commit before the family's backward paths were unified
in nnops.py, with the recorder of tests/op_trace.py as it stands:

    python tests/op_trace_conv_cases.py | xz -9e > tests/golden/op_trace_conv.txt.xz
"""
import pytest

import op_trace
from op_trace import conv_bn, fmap, nn, nnops

B, H, W = 2, 6, 5
ROUTE_ENV = ("PK_CONV1X1_BN", "PK_CONV1X1_BN_MIN_ROWS", "PK_CONV1X1_BN_MAX_GRID", "PK_BN_OUT1X1", "PK_BN_OUT1X1_MIN_ROWS", "PK_BN_OUT1X1_MAX_GRID")
RECOMPUTE = {"PK_CONV1X1_BN_MIN_ROWS": "1"}
FUSED_OUT = {"PK_BN_OUT1X1_MIN_ROWS": "1"}

CASES = {}      # name -> (build, options), as op_trace.CASES


def case(name, grad=True, env=None):
    def deco(build):
        CASES[name] = (build, dict(grad=grad, env=env or {}))
        return build
    return deco


@case("stem_input_grad")
def _stem():
    m = nn.Sequential(*conv_bn(3, 16, 3, 2))
    return m, dict(x=fmap(B, H, W, 8)), lambda m, i, drop: nnops.conv_bn_act(i["x"], m[0], m[1], True, None, True)


def _deconv_eval(k):
    @case(f"deconv_k{k}_eval_grad")
    def build():
        m = nn.Sequential(nn.ConvTranspose2d(16, 24, k, 2, (k - 1) // 2, bias=False), nn.BatchNorm2d(24))
        return m, dict(x=fmap(B, H, W, 16)), lambda m, i, drop: nnops.deconv_bn_relu(i["x"], m[0], m[1], False)


_deconv_eval(2)
_deconv_eval(4)


def _recompute(name, relu, residual, grad=True):
    @case(name, grad=grad, env=RECOMPUTE)
    def build():
        m = nn.Sequential(*conv_bn(64, 256, 1))
        ins = dict(x=fmap(B, H, W, 64, grad))
        if residual:
            ins["res"] = fmap(B, H, W, 256, grad)
        return m, ins, lambda m, i, drop: nnops.conv_bn_act(i["x"], m[0], m[1], relu, i.get("res"), True)


_recompute("recompute_relu_res", True, True)
_recompute("recompute_relu", True, False)
_recompute("recompute_plain", False, False)
_recompute("recompute_train_no_grad", True, True, grad=False)


@case("recompute_after_two_stored", env=RECOMPUTE)
def _chain():
    m = nn.Sequential(*conv_bn(64, 64, 1), *conv_bn(64, 64, 3), *conv_bn(64, 256, 1))

    def run(m, i, drop):
        y = nnops.conv_bn_act(i["x"], m[0], m[1], True, None, True)
        y = nnops.conv_bn_act(y, m[2], m[3], True, None, True)
        return nnops.conv_bn_act(y, m[4], m[5], True, i["res"], True)
    return m, dict(x=fmap(B, H, W, 64), res=fmap(B, H, W, 256)), run


def _branch(name, C, N, softplus, env):
    @case(name, env=env)
    def build():
        m = nn.Sequential(*conv_bn(16, C, 3), nn.Conv2d(C, N, 1))
        return m, dict(x=fmap(B, H, W, 16)), lambda m, i, drop: nnops.conv_bn_act_out(i["x"], m[0], m[1], m[2], softplus, True)


_branch("branch_256_17", 256, 17, False, FUSED_OUT)
_branch("branch_256_34", 256, 34, False, FUSED_OUT)
_branch("branch_128_17_softplus", 128, 17, True, FUSED_OUT)
_branch("branch_128_17_softplus_route_off", 128, 17, True, dict(FUSED_OUT, PK_BN_OUT1X1="0"))


@case("head_out_24")
def _head():
    m = nn.Sequential(nn.Conv2d(16, 24, 1))
    return m, dict(x=fmap(B, H, W, 16)), lambda m, i, drop: nnops.head_out(i["x"], m[0], False)


def trace(name, regime, mp):
    """op_trace.trace of one case of this module: the route switches start unset, the case is in op_trace.CASES for this trace only."""
    for k in ROUTE_ENV:
        mp.delenv(k, raising=False)
    mp.setitem(op_trace.CASES, name, CASES[name])
    return op_trace.trace(name, regime, mp)


if __name__ == "__main__":
    for _name in CASES:
        for _regime in op_trace.REGIMES:
            with pytest.MonkeyPatch.context() as _mp:
                print(f"== {_name}/{_regime}")
                print("\n".join(trace(_name, _regime, _mp)))
