"""Which kernels, grids and arguments every problem gets from the library status, target, decode and input units (pk_status.hip,
pk_target.hip, pk_decode.hip, pk_input.hip) and from the entries next to them in pk_layout.hip (pk_rows_by_map, pk_drop_path_f32),
pk_motion.hip (pk_temporal_smooth, pk_nms_pose) and pk_eval.hip (pk_pose_records), pinned against a recorded fixture.

tests/launch_recorder_post.hip compiles the seven units for the host with the launch macro replaced by a printer and drives each of the
23 extern "C" entries over the values at which its launch rule or an argument check can go wrong: one and 34 maps and a 46341 x 46341
map for the one-workgroup-per-map entries, 1 / 255 / 256 / 257 lanes for the one-lane-per-map entries, totals around a workgroup,
around the 4096-workgroup cap and beyond 32 bits for the grid-stride entries, every mode, kernel size, scale count and window the
entries tell apart, a lookup table one entry too short, crops of 255 / 256 / 257 pixels and 2370 x 2370, a workspace one byte too
small, a null in each pointer, misaligned outputs, pairs of faults (which check comes first).  The library's own error state is
compiled in, so the error text is what pk_last_error_string gives back.  No device is opened, on any machine.  Its output must equal
tests/golden/launch_routes_post.txt.xz line for line.  The fixture was recorded from the single unit pk_target_decode.hip all of this
was split from (commit d5b3355), where every entry carried its own copy of the checks and the grid expression:

    git show d5b3355:infantposeestimation_gaussianbias_amd/csrc/pk_target_decode.hip > /tmp/pk_target_decode.hip
    hipcc --offload-host-only -O1 -std=c++17 -w -I infantposeestimation_gaussianbias_amd/csrc -DPK_POST_SINGLE_UNIT='"/tmp/pk_target_decode.hip"' \
        tests/launch_recorder_post.hip -o /tmp/launch_recorder_post
    /tmp/launch_recorder_post | xz -9e > tests/golden/launch_routes_post.txt.xz

(575 lines; the old unit is included as it was, error state and all, and still compiles against the headers of this tree).  A
deliberate change of a launch rule or a check regenerates it from the units as they are:

    hipcc --offload-host-only -O1 -std=c++17 -w tests/launch_recorder_post.hip -o /tmp/launch_recorder_post
    /tmp/launch_recorder_post | xz -9e > tests/golden/launch_routes_post.txt.xz
"""
import lzma
import os
import subprocess

import pytest

from test_launch_routes import ROOT, _hipcc


def test_every_post_launch_matches_the_recorded_routes(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder_post")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder_post.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_routes_post.txt.xz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 550          # the fixture itself is whole
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
