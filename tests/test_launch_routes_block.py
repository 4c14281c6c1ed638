"""Which kernels, grids, LDS sizes and launcher-filled argument blocks every problem gets from pk_block_mlp.hip, pk_block_attn.hip and
pk_attn.hip, pinned against a recorded fixture.

tests/launch_recorder_block.hip compiles the three units for the host with the launch macro replaced by a printer and drives every
extern "C" entry over the values at which its launch rule can go wrong: the row counts around the workgroup caps of the fused MLP
kernels, the staged-once / streamed switch and the 160-workgroup rule of the wide forward, the window caps of the fused attention
kernels, the four head-dimension arms and the group rule of the window-attention core, the 32-bit refusals, a null and an 8-byte
offset in each pointer, pairs of faults (which check comes first).  No device is opened, on any machine.  Its output must equal
tests/golden/launch_routes_block.txt.xz line for line.  The fixture was recorded from the single unit pk_block.hip the two block units
were split from (commit cc07bdc), where every entry carried its own copy of the argument checks and the grid rule:

    git show cc07bdc:infantposeestimation_gaussianbias_amd/csrc/pk_block.hip > /tmp/pk_block.hip
    hipcc --offload-host-only -O1 -std=c++17 -w -I infantposeestimation_gaussianbias_amd/csrc -DPK_BLOCK_SINGLE_UNIT='"/tmp/pk_block.hip"' \
        tests/launch_recorder_block.hip -o /tmp/launch_recorder_block
    /tmp/launch_recorder_block | xz -9e > tests/golden/launch_routes_block.txt.xz

(1 036 lines; the old unit still compiles against the headers of this tree and gives the same lines).  A deliberate change of a launch rule (a new cap, a new width)
regenerates it from the units as they are:

    hipcc --offload-host-only -O1 -std=c++17 -w tests/launch_recorder_block.hip -o /tmp/launch_recorder_block
    /tmp/launch_recorder_block | xz -9e > tests/golden/launch_routes_block.txt.xz
"""
import lzma
import os
import subprocess

import pytest

from test_launch_routes import ROOT, _hipcc


def test_every_block_launch_matches_the_recorded_routes(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder_block")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder_block.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_routes_block.txt.xz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 1000          # the fixture itself is whole
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
