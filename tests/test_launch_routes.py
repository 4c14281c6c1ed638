"""Which kernel, tile, grid and slice count every shape gets from pk_igemm.hip and pk_wgrad.hip, pinned against a recorded fixture.

tests/launch_recorder.hip compiles the two units for the host with the launch macro replaced by a printer and drives the real entry
points over a sweep of shapes, options and routing switches (no device is opened, on any machine).  Its output must equal
tests/golden/launch_routes.txt.xz line for line.  The fixture was recorded from the single-unit library before the routing was gathered
into igemm_route / wgrad_route; a deliberate routing change (a new threshold, a new tile) regenerates it:

    hipcc --offload-host-only -O1 -std=c++17 tests/launch_recorder.hip -o /tmp/launch_recorder
    /tmp/launch_recorder | xz -9e > tests/golden/launch_routes.txt.xz
"""
import lzma
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def test_every_launch_matches_the_recorded_routes(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found: the launch recorder cannot be built")
    exe = str(tmp_path / "launch_recorder")
    build = subprocess.run([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-w", os.path.join(ROOT, "tests", "launch_recorder.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PK_CONV")}          # the recorder sets the routing switches itself
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_routes.txt.xz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 100000          # the fixture itself is whole
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  recorded: {w}\n  now:      {g}"
    assert len(got) == len(want), f"{len(got)} lines, fixture has {len(want)}"
