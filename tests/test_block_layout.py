"""The layout of a call's device block (csrc/block_layout.h, used by every capi_<stage>.hip through capi_ctx.h's
Block): tests/cpp/block_layout.cpp declares the pieces of svo_klt_track, svo_bundle_adjust, svo_pose_optimize and
FeatureAlignment as the entry points do and compares offsets, region ends, total and copy list with the numbers the
hand-written offset arithmetic gave.  Host-only: the header needs no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_layout_matches_the_hand_written_offsets(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "block_layout")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "semi-direct-visual-odometry_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "block_layout.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr
