#!/usr/bin/env python3
"""Ren SDF tracker timings at 640x480 (tests/ren_cases.py inputs: the ITMVoxel_s hash scene fused from three frames of the parity
trajectory at 5 mm, the depth frame one step further, 307 200 points): microseconds per F evaluation (energy only), per G
evaluation (energy + gradient + Hessian in one pass), evaluations per TrackCamera from the previous frame's pose, milliseconds per
TrackCamera and the TrackCamera rate it allows, and the closed loop: ITMMainEngine_HIP with TRACKER_REN on ITMVoxel_s hash
(tests/cpp/ren_engine_demo.cpp, view building + tracking + fusion + ray cast per frame, median over the frames after the first).
One JSON line.  Run on the GPU:  python tools/ren_tracker_bench.py [reps]"""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import itm_testlib as T  # noqa: E402
import ren_cases as RC  # noqa: E402
from infinitam_amd import capi  # noqa: E402
from infinitam_amd.capi import RenEval  # noqa: E402


def main(reps=200):
    be = T.hip_backend()
    sc = RC.SCENES["vga_hash_s"]
    ses = T.Session(be, sc)
    for k in range(sc.frames):
        ses.frame(k)
    d = be.to_backend(RC.depth(sc))
    start = np.asarray(RC.starts()["previous"], np.float32)
    view = capi.View(d, sc.w, sc.h, M_d=start, intr_d=sc.intr()).struct()
    h = C.c_void_p()
    be.check(be.fn["ren_tracker_create"](C.byref(h)), "create")
    be.check(be.fn["ren_tracker_prepare"](h, C.byref(view), None, None), "prepare")
    inv = np.ascontiguousarray(RC.eval_inv_poses(sc)["previous"], np.float32)
    pinv = inv.ctypes.data_as(C.POINTER(C.c_float))
    scene = C.c_void_p(ses.scene.h)
    out = RenEval()
    res = {"w": sc.w, "h": sc.h, "points": sc.w * sc.h}
    for g, key in ((0, "us_per_F"), (1, "us_per_G")):
        for _ in range(10):
            be.check(be.fn["ren_tracker_evaluate"](h, scene, pinv, g, C.byref(out), None), "evaluate")
        t0 = time.perf_counter()
        for _ in range(reps):
            be.fn["ren_tracker_evaluate"](h, scene, pinv, g, C.byref(out), None)
        res[key] = round((time.perf_counter() - t0) / reps * 1e6, 1)
    res["valid_points"] = out.noValidPoints
    M = (C.c_float * 16)()
    n = C.c_int()
    for _ in range(3):
        be.check(be.fn["ren_tracker_track_camera"](h, scene, C.byref(view), M, C.byref(n), None), "track")
    k = max(5, reps // 10)
    t0 = time.perf_counter()
    for _ in range(k):
        be.fn["ren_tracker_track_camera"](h, scene, C.byref(view), M, C.byref(n), None)
    ms = (time.perf_counter() - t0) / k * 1e3
    res.update(evaluations_per_track=n.value, ms_per_track=round(ms, 3), tracks_per_s=round(1e3 / ms, 1))
    be.fn["ren_tracker_destroy"](h)
    ses.close()
    import test_ren_engine as E
    import subprocess
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "seq.bin")
        E.write_sequence(path)
        txt = subprocess.run([E.build_demo(), path, "s"], check=True, capture_output=True, text=True, timeout=600).stdout
        rows = [json.loads(line) for line in txt.splitlines() if line.startswith("{")]
    us = float(np.median([r["us"] for r in rows[1:]]))
    res.update(closed_loop_us_per_frame=round(us, 1), closed_loop_frames_per_s=round(1e6 / us, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
