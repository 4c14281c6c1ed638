"""The conv + BatchNorm family's launches, queued reductions and autograd returns on the routes tests/golden/op_trace.txt.xz does not
hold, pinned line for line against tests/golden/op_trace_conv.txt.xz (tests/op_trace_conv_cases.py says what the cases are and how the
fixture was recorded).  No device is opened on any machine."""
import lzma
import os

import pytest
import torch

import op_trace
import op_trace_conv_cases as cases

_FIXTURE = []


def recorded():
    if not _FIXTURE:
        with lzma.open(os.path.join(op_trace.ROOT, "tests", "golden", "op_trace_conv.txt.xz"), "rt") as f:
            _FIXTURE.append(op_trace.sections(f.read()))
    return _FIXTURE[0]


def test_the_fixture_holds_every_case_and_regime():
    assert sorted(recorded()) == sorted(f"{c}/{r}" for c in cases.CASES for r in op_trace.REGIMES)


@pytest.mark.parametrize("regime", op_trace.REGIMES)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_conv_family_trace_equals_the_recorded_one(name, regime, monkeypatch):
    got, want = cases.trace(name, regime, monkeypatch), recorded()[f"{name}/{regime}"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"


def test_a_skip_gradient_that_was_never_produced_raises(monkeypatch):
    """the first conv of a residual block whose last conv has not run its backward: the hand-over slot is empty"""
    nnops = op_trace.nnops
    op_trace.install(monkeypatch, op_trace.Recorder())
    monkeypatch.setattr(nnops, "call", lambda name, *args: None)          # nothing is recorded here: the launches go nowhere
    m =op_trace.nn.Sequential(*op_trace.conv_bn(16, 16, 3))
    with torch.enable_grad(), nnops.use_weights(m):
        y = nnops.conv_bn_act(op_trace.fmap(2, 6, 5, 16), m[0], m[1], True, None, True, skip_in=nnops.SkipGrad())
        with pytest.raises(op_trace._lib.PoseKernelError, match="residual block backward out of order: the skip gradient has not been produced yet"):
            y.backward(torch.zeros_like(y))
    nnops.discard_deferred()
