#!/usr/bin/env python3
"""Colour tracker timings at 640x480 (tests/colour_cases.py inputs: the textured scene, a 320 x 240 point cloud):
microseconds per evaluation (cost + gradient + Hessian in one pass, and cost only) per level, evaluations per TrackCamera,
microseconds per TrackCamera and the TrackCamera rate it allows, and the closed loop: ITMMainEngine_HIP with TRACKER_COLOR +
useColourTracker on ITMVoxel_f_rgb (tests/cpp/colour_engine_demo.cpp, view building + tracking + fusion + point cloud per frame,
median over the frames after the first).  One JSON line.  Run on the GPU:  python tools/colour_tracker_bench.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import colour_cases as CC  # noqa: E402
import itm_testlib as T  # noqa: E402
from infinitam_amd import capi  # noqa: E402
from infinitam_amd.capi import ColourEval, TrackerConfig  # noqa: E402


def main(reps=200):
    be = T.hip_backend()
    loc, col = CC.cloud()
    dl, dc = be.to_backend(loc), be.to_backend(col)
    n = loc.shape[0]
    img = CC.frame(CC.motions()["both"][0])
    rgb = be.to_backend(img)
    dummy = be.to_backend(np.zeros((CC.H, CC.W), np.float32))
    view = capi.View(dummy, CC.W, CC.H, intr_d=CC.INTR, rgb=rgb, w_rgb=CC.W, h_rgb=CC.H, intr_rgb=CC.INTR).struct()
    h = C.c_void_p()
    be.check(be.fn["colour_tracker_create"](C.byref(h)), "create")
    be.check(be.fn["colour_tracker_prepare"](h, C.byref(view), CC.LEVELS, None), "prepare")
    pose = (C.c_float * 16)(*[float(x) for x in CC.IDENTITY])
    out = ColourEval()
    res = {"w": CC.W, "h": CC.H, "points": n}
    for gh, key in ((1, "us_per_eval_fused"), (0, "us_per_eval_cost_only")):
        per = []
        for lv in range(CC.LEVELS):
            for _ in range(10):
                be.check(be.fn["colour_tracker_evaluate"](h, lv, dl.ptr, dc.ptr, n, pose, 3, gh, C.byref(out), None), "eval")
            t0 = time.perf_counter()
            for _ in range(reps):
                be.fn["colour_tracker_evaluate"](h, lv, dl.ptr, dc.ptr, n, pose, 3, gh, C.byref(out), None)
            per.append(round((time.perf_counter() - t0) / reps * 1e6, 1))
        res[key] = per
    cfg = TrackerConfig.default()
    M = (C.c_float * 16)()
    for _ in range(5):
        be.check(be.fn["colour_tracker_track_camera"](h, C.byref(cfg), C.byref(view), None, dl.ptr, dc.ptr, n, M, None), "track")
    t0 = time.perf_counter()
    k = 50
    for _ in range(k):
        be.fn["colour_tracker_track_camera"](h, C.byref(cfg), C.byref(view), None, dl.ptr, dc.ptr, n, M, None)
    us = (time.perf_counter() - t0) / k * 1e6
    ev = C.c_int()
    be.check(be.fn["colour_tracker_evaluations"](h, C.byref(ev)), "evaluations")
    res.update(evaluations_per_track=ev.value, us_per_track=round(us, 1), tracks_per_s=round(1e6 / us, 1))
    be.fn["colour_tracker_destroy"](h)
    import tempfile
    import test_colour_engine as E
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "seq.bin")
        E.write_sequence(path)
        rows = E.run_loop(path, "f_rgb")
    us = float(np.median([r["us"] for r in rows[1:]]))
    res.update(closed_loop_us_per_frame=round(us, 1), closed_loop_frames_per_s=round(1e6 / us, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
