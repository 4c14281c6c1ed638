"""The op layer's launches, queued reductions and autograd returns, pinned against a trace recorded before its gradient-destination
and slab-reduction paths were unified (tests/op_trace.py says what is recorded and how the fixture is regenerated).  No device is
opened on any machine: the C-ABI chokepoints are replaced by a recorder, so a case is a few milliseconds of host code."""
import lzma
import os

import pytest

import op_trace

_FIXTURE = []


def recorded():
    if not _FIXTURE:
        with lzma.open(os.path.join(op_trace.ROOT, "tests", "golden", "op_trace.txt.xz"), "rt") as f:
            _FIXTURE.append(op_trace.sections(f.read()))
    return _FIXTURE[0]


def test_the_fixture_holds_every_case_and_regime():
    assert sorted(recorded()) == sorted(f"{c}/{r}" for c in op_trace.CASES for r in op_trace.REGIMES)


@pytest.mark.parametrize("regime", op_trace.REGIMES)
@pytest.mark.parametrize("name", list(op_trace.CASES))
def test_op_layer_trace_equals_the_recorded_one(name, regime, monkeypatch):
    got, want = op_trace.trace(name, regime, monkeypatch), recorded()[f"{name}/{regime}"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
