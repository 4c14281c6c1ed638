"""Which kernels, grids and arguments every problem gets from the analysis units, pinned against a recorded fixture: pk_pck,
pk_motion_stats and pk_position_histogram of pk_motion.hip, pk_motion_spectrum of pk_spectrum.hip, pk_pose_rescore and pk_oks_nms of
pk_nms.hip, pk_coco_kpt_oks and pk_coco_kpt_eval (with its workspace query) of pk_eval.hip, and pk_draw_shapes, pk_heatmap_overlay and
pk_heatmap_overlay_patches (with their workspace queries) of pk_draw.hip.

tests/launch_recorder_analysis.hip compiles the five units and pk_status.hip for the host with the launch macro replaced by a printer
and drives the ten launching entries and three queries over the values at which a launch rule or an argument check can go wrong: 1 and
34 joints, S K at 2^31 - 1 and beyond, 1 / 16 / 17 thresholds, 16384 and 16385 histogram bins, 1 / 64 / 65 / 16384 / 16385 spectrum bins
(the ceil(F / 64) grid), a band that ends at N / 2 and one bin beyond, N = 2 and 2^30 + 1, window 2, K = 64 and 65, soft mode with
thr = 0 and max_dets = 0, NaN thresholds, 255 / 256 / 257 poses for the one-lane-per-pose entry, 64 and 65 curves, overlay planes of
1 x 1, 2047, 2048 and 2049 pixels and on each side of the 256-workgroup cap, 65535 and 65536 images, sizes at and beyond 8192,
workspace queries that overflow, a null in each pointer, pairs of faults (which check comes first).  The library's own error state is
compiled in, so the error text is what pk_last_error_string gives back.  No device is opened, on any machine.  Its output must equal
tests/golden/launch_routes_analysis.txt.xz line for line.  The fixture was recorded from the units of commit 2f2f9ac, the last one in
which pk_motion.hip, pk_spectrum.hip and pk_input.hip each carried a copy of the workgroup reduction and the frame rule and every
sequence entry its own shape check:

    mkdir /tmp/parent && git archive 2f2f9ac infantposeestimation_gaussianbias_amd/csrc include | tar -x -C /tmp/parent
    hipcc --offload-host-only -O1 -std=c++17 -w -DPK_ANALYSIS_CSRC=/tmp/parent/infantposeestimation_gaussianbias_amd/csrc \
        tests/launch_recorder_analysis.hip -o /tmp/launch_recorder_analysis
    /tmp/launch_recorder_analysis | xz -9e > tests/golden/launch_routes_analysis.txt.xz

(688 lines).  A deliberate change of a launch rule or a check regenerates it from the units as they are:

    hipcc --offload-host-only -O1 -std=c++17 -w tests/launch_recorder_analysis.hip -o /tmp/launch_recorder_analysis
    /tmp/launch_recorder_analysis | xz -9e > tests/golden/launch_routes_analysis.txt.xz
"""
import lzma
import os
import subprocess

import pytest

from test_launch_routes import ROOT, _hipcc


def test_every_analysis_launch_matches_the_recorded_routes(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder_analysis")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder_analysis.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_routes_analysis.txt.xz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 650          # the fixture itself is whole
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
