"""The colour tracker behind the engine interfaces: ITMMainEngine_HIP with TRACKER_COLOR and useColourTracker = true
(include/itm_hip_engines.hpp: ITMColorTracker_HIP + ITMColorTrackerAdapter), driven by tests/cpp/colour_engine_demo.cpp, and the
C-ABI path that takes the point count from the render state create_point_cloud wrote.

  * closed loop, no outside poses: 15 frames of the textured sphere + wall (tests/colour_cases.py, 2 mm and 0.15 degrees per frame)
    on ITMVoxel_f_rgb and ITMVoxel_s_rgb; each frame is tracked against the point cloud rendered from the previous tracked pose, so
    errors accumulate.  Every frame's mean reprojection error of the scene (tracked vs true pose) stays below LOOP_PX pixels and
    below a quarter of what the untracked camera reaches by the last frame (measured on an MI355X: 1.0 px after the first tracked
    frame, growing by ~0.2 px per frame to 3.4 px on both voxel types, against 33.6 px untracked; the pose error itself lies along
    the sideways-move / yaw direction this scene barely tells apart, 1.1e-2 in max |R - R_true|);
  * a voxel type without colour is refused (ITMLibSettings.cpp:81) -- on the host, before anything is allocated;
  * track_camera with the render state (count read on the device) returns the same bits as with the count passed explicitly.
"""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import colour_cases as CC
import itm_testlib as T
from infinitam_amd import capi, synth
from infinitam_amd.capi import TrackerConfig

SRC = os.path.join(T.ROOT, "tests", "cpp", "colour_engine_demo.cpp")
EXE = os.path.join(T.ROOT, "tests", "cpp", "colour_engine_demo")
LOOP_PX = 4.0


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
        for k in range(frames):
            f.write(np.ascontiguousarray(CC.frame(CC.loop_pose(k))).tobytes())


def run_loop(path, voxel, timeout=600):
    out = subprocess.run([build_demo(), path, voxel], check=True, capture_output=True, text=True, timeout=timeout).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def test_colourless_voxel_type_is_refused():
    r = subprocess.run([build_demo(), "--colourless"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("refused: Color tracker requires a voxel type with color information"), r.stdout + r.stderr


def reprojection_px(M_track, M_true):
    """Mean image distance (pixels) between where the tracked and the true pose put the surface points the true camera sees
    (a 40 x 30 grid): what the photometric cost measures.  A sideways move and a yaw shift this distant, nearly frontal scene
    almost alike, so the pose error itself splits between the two along that direction; its image is what tracking fixes."""
    X = synth.surface_points(40, 30, M_true, tuple(v / 16.0 for v in CC.INTR)).reshape(-1, 3)
    fx, fy, cx, cy = CC.INTR

    def project(M16):
        M = CC.mat(M16)
        q = X @ M[:3, :3].T + M[:3, 3]
        return np.stack([fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy], -1)
    return float(np.linalg.norm(project(M_track) - project(M_true), axis=1).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", ["f_rgb", "s_rgb"])
def test_closed_loop_follows_the_trajectory(tmp_path, voxel):
    path = str(tmp_path / "seq.bin")
    write_sequence(path)
    rows = run_loop(path, voxel)
    assert len(rows) == CC.LOOP_FRAMES
    tracked = [reprojection_px(np.array(r["M"], np.float32), CC.loop_pose(k)) for k, r in enumerate(rows)]
    untracked = [reprojection_px(CC.loop_pose(0), CC.loop_pose(k)) for k in range(len(rows))]
    worst_r = max(np.abs(CC.mat(np.array(r["M"], np.float32))[:3, :3] - CC.mat(CC.loop_pose(k))[:3, :3]).max() for k, r in enumerate(rows))
    print(f"colour loop {voxel}: reprojection error per frame (px) {np.round(tracked, 2).tolist()}, untracked at the end "
          f"{untracked[-1]:.1f} px, worst |R - R_true| {worst_r:.2e}, median ProcessFrame {np.median([r['us'] for r in rows[1:]]):.0f} us")
    assert max(tracked) < LOOP_PX and max(tracked) < 0.25 * untracked[-1], (tracked, untracked[-1])


@pytest.mark.gpu
def test_track_camera_reads_the_point_count_from_the_render_state():
    hip = T.hip_backend()
    s = hip.create_scene(capi.VOXEL_F_RGB, capi.INDEX_HASH, capi.default_params(voxelSize=0.005))
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((CC.W, CC.H))
    depth = hip.to_backend((CC.raw_depth_mm(CC.IDENTITY).astype(np.float32) * np.float32(0.001)).astype(np.float32))
    rgb0 = hip.to_backend(np.ascontiguousarray(CC.frame(CC.IDENTITY)))
    v0 = capi.View(depth, CC.W, CC.H, intr_d=CC.INTR, rgb=rgb0, w_rgb=CC.W, h_rgb=CC.H, intr_rgb=CC.INTR)
    s.reco.AllocateSceneFromDepth(v0, rs)
    s.reco.IntegrateIntoScene(v0, rs)
    loc = capi.DevBuffer(hip, CC.W * CC.H * 16, np.float32, (CC.W * CC.H, 4))
    col = capi.DevBuffer(hip, CC.W * CC.H * 16, np.float32, (CC.W * CC.H, 4))
    s.vis.CreateExpectedDepths(CC.IDENTITY, CC.INTR, rs)
    s.vis.CreatePointCloud(v0, rs, loc, col, skipPoints=True)
    n = s.counters(rs)["noTotalPoints"]
    assert n > 10000
    rgb1 = hip.to_backend(np.ascontiguousarray(CC.frame(CC.motions()["yaw1"][0])))
    v1 = capi.View(depth, CC.W, CC.H, intr_d=CC.INTR, rgb=rgb1, w_rgb=CC.W, h_rgb=CC.H, intr_rgb=CC.INTR).struct()
    cfg = TrackerConfig.default()
    h = C.c_void_p()
    hip.check(hip.fn["colour_tracker_create"](C.byref(h)), "create")
    try:
        a, b = (C.c_float * 16)(), (C.c_float * 16)()
        hip.check(hip.fn["colour_tracker_track_camera"](h, C.byref(cfg), C.byref(v1), C.c_void_p(rs.h), loc.ptr, col.ptr, 0, a, None), "rs")
        hip.check(hip.fn["colour_tracker_track_camera"](h, C.byref(cfg), C.byref(v1), None, loc.ptr, col.ptr, n, b, None), "count")
    finally:
        hip.fn["colour_tracker_destroy"](h)
    np.testing.assert_array_equal(np.array(a[:]), np.array(b[:]))
    assert not np.array_equal(np.array(a[:]), CC.IDENTITY)          # it did track
