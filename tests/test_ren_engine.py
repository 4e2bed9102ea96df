"""The Ren SDF tracker behind the engine interfaces: ITMMainEngine_HIP with TRACKER_REN (include/itm_hip_engines.hpp:
ITMRenTracker_HIP + ITMRenTrackerAdapter), driven by tests/cpp/ren_engine_demo.cpp.

Closed loop, no outside poses: 15 depth frames of the textured sphere + wall (tests/colour_cases.py, the camera moves 2 mm sideways
and yaws 0.15 degrees per frame) on ITMVoxel_s and ITMVoxel_f with the hash index and ITMVoxel_s dense.  Every frame starts from the
previous tracked pose -- a small pose error the tracker has to remove -- and is registered against the TSDF the earlier frames fused
at their tracked poses, so errors accumulate.  From the third frame on, every frame's mean reprojection error of the scene (tracked
vs true pose) stays below LOOP_RATIO of the untracked camera's at that frame.

The Ren tracker removes only part of each frame's motion on this scene: its robust energy and the 1e-4 relative-decrease stop end
the loop early, as they do in the reference (tests/golden/g_ren_tracker.json, "previous": a 10 mm start error ends 5.2 mm off).
Measured on an MI355X: the error grows to 12.3 px (ITMVoxel_s hash) and 15.4 px (ITMVoxel_s dense) by frame 15, against 33.6 px
untracked; the photometric tracker, whose cost sees the texture, stays below 4 px on the same sequence (tests/test_colour_engine.py).
"""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import colour_cases as CC
import itm_testlib as T
from test_colour_engine import reprojection_px

SRC = os.path.join(T.ROOT, "tests", "cpp", "ren_engine_demo.cpp")
EXE = os.path.join(T.ROOT, "tests", "cpp", "ren_engine_demo")
LOOP_RATIO = 0.6


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), SRC, "-o", EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return EXE


def write_sequence(path, frames=CC.LOOP_FRAMES):
    with open(path, "wb") as f:
        f.write(struct.pack("3i", CC.W, CC.H, frames))
        f.write(np.array(CC.INTR, np.float32).tobytes())
        for k in range(frames):
            f.write(CC.raw_depth_mm(CC.loop_pose(k)).tobytes())


def test_demo_builds():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", ["s", "f", "s_dense"])
def test_closed_loop_follows_the_trajectory(tmp_path, voxel):
    path = str(tmp_path / "seq.bin")
    write_sequence(path)
    out = subprocess.run([build_demo(), path, voxel], check=True, capture_output=True, text=True, timeout=600).stdout
    rows = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    assert len(rows) == CC.LOOP_FRAMES
    tracked = [reprojection_px(np.array(r["M"], np.float32), CC.loop_pose(k)) for k, r in enumerate(rows)]
    untracked = [reprojection_px(CC.loop_pose(0), CC.loop_pose(k)) for k in range(len(rows))]
    print(f"Ren loop {voxel}: reprojection error per frame (px) {np.round(tracked, 2).tolist()}, untracked at the end "
          f"{untracked[-1]:.1f} px, median ProcessFrame {np.median([r['us'] for r in rows[1:]]):.0f} us")
    ratios = [t / u for t, u in zip(tracked[2:], untracked[2:])]
    assert max(ratios) < LOOP_RATIO, (np.round(ratios, 3).tolist(), tracked, untracked)
