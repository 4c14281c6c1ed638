"""Which kernels, grids and launcher-computed arguments every problem gets from pk_bn.hip, pk_ln.hip, pk_exchange.hip and pk_layout.hip,
pinned against a recorded fixture.

tests/launch_recorder_norm.hip compiles the four units for the host with the launch macro replaced by a printer and drives every
extern "C" entry over the values at which its launch rule can go wrong: the workgroup rule of the fused BatchNorm kernels, the fused /
three-launch switch, the block caps and the 32-bit refusal of the chunk grids, the LayerNorm lane switch, the up-sampling split, group
sizes and bad members, a null in each required pointer (no device is opened, on any machine).  Its output must equal
tests/golden/launch_routes_norm.txt.xz line for line.  The fixture was recorded from the single unit pk_norm.hip the four were split
from (commit bfa546a), where the single and the grouped entries each carried their own copy of these rules:

    git show bfa546a:infantposeestimation_gaussianbias_amd/csrc/pk_norm.hip > /tmp/pk_norm.hip
    hipcc --offload-host-only -O1 -std=c++17 -I infantposeestimation_gaussianbias_amd/csrc -DPK_NORM_SINGLE_UNIT='"/tmp/pk_norm.hip"' \
        tests/launch_recorder_norm.hip -o /tmp/launch_recorder_norm

A deliberate change of a launch rule (a new threshold, a folded launch) regenerates it from the units as they are:

    hipcc --offload-host-only -O1 -std=c++17 tests/launch_recorder_norm.hip -o /tmp/launch_recorder_norm
    /tmp/launch_recorder_norm | xz -9e > tests/golden/launch_routes_norm.txt.xz
"""
import lzma
import os
import subprocess

import pytest

from test_launch_routes import ROOT, _hipcc


def test_every_norm_launch_matches_the_recorded_routes(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder_norm")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder_norm.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_routes_norm.txt.xz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 14000          # the fixture itself is whole
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
