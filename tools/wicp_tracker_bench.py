#!/usr/bin/env python3
"""Weighted ICP tracker timings at 160x120 and 640x480 (tests/wicp_cases.py inputs: ICP maps of three fused frames, the next depth
frame and its sigmaZ image): host microseconds per weighted evaluation (itm_tracker_weighted_g_and_h, launch to sums) on every level
of the default 5-level hierarchy (3 levels at 160x120), milliseconds per TrackCamera from the previous frame's pose, and the number
of evaluations that TrackCamera makes (the same loop driven through itm_debug_wicp_track with the GPU evaluation as its evaluator).
One JSON line.  Kernel times: run under rocprofv3 --kernel-trace --stats.  Run on the GPU:  python tools/wicp_tracker_bench.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import itm_testlib as T  # noqa: E402
import wicp_cases as WC  # noqa: E402
from infinitam_amd import capi  # noqa: E402
from infinitam_amd.capi import TrackerConfig, TrackerGH  # noqa: E402

EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(TrackerGH))


def fptr(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def one_size(be, oracle, sc, cfg, reps):
    points, normals, M_d, depth, sigma = WC.build(oracle, sc)
    levels = cfg.noHierarchyLevels
    dp, dn, dd, ds = (be.to_backend(a) for a in (points, normals, depth, sigma))
    pd = [be.to_backend(a) for a in WC.numpy_pyramid(depth, levels)]
    pw = [be.to_backend(a) for a in WC.numpy_pyramid(sigma, levels)]
    shapes = [a.shape for a in WC.numpy_pyramid(depth, levels)]
    h = C.c_void_p()
    be.check(be.fn["tracker_create"](C.byref(h)), "create")
    inv = np.ascontiguousarray(WC.eval_inv_poses(M_d)["at_previous"], np.float32)
    thr = WC.level_thresholds(levels, cfg.distThresh)
    res = {"size": f"{sc.w}x{sc.h}", "eval_us": {}}

    def evaluate(level, mode, inv_pose, dist, out):
        hl, wl = shapes[level]
        intr = np.array(sc.intr(), np.float32) * np.float32(0.5 ** level)
        return be.fn["tracker_weighted_g_and_h"](h, pd[level].ptr, pw[level].ptr, wl, hl, fptr(intr), dp.ptr, dn.ptr, sc.w, sc.h,
                                                 fptr(sc.intr()), inv_pose, fptr(M_d), dist, mode, out, None)

    for l in range(levels):
        mode = cfg.trackingRegime[l]
        o = TrackerGH()
        for _ in range(10):
            be.check(evaluate(l, mode, fptr(inv), thr[l], C.byref(o)), "eval")
        t0 = time.perf_counter()
        for _ in range(reps):
            evaluate(l, mode, fptr(inv), thr[l], C.byref(o))
        res["eval_us"][f"level{l}_mode{mode}"] = round((time.perf_counter() - t0) / reps * 1e6, 2)
    view = capi.View(dd, sc.w, sc.h, M_d=M_d, intr_d=sc.intr()).struct()
    out = (C.c_float * 16)()
    for _ in range(5):
        be.check(be.fn["tracker_weighted_track_camera"](h, C.byref(cfg), C.byref(view), ds.ptr, dp.ptr, dn.ptr, fptr(M_d), out, None), "track")
    t0 = time.perf_counter()
    for _ in range(reps // 4 or 1):
        be.fn["tracker_weighted_track_camera"](h, C.byref(cfg), C.byref(view), ds.ptr, dp.ptr, dn.ptr, fptr(M_d), out, None)
    res["track_camera_ms"] = round((time.perf_counter() - t0) / (reps // 4 or 1) * 1e3, 4)
    calls = []
    cb = EVAL_FN(lambda user, level, mode, ip, dist, o: calls.append(level) or evaluate(level, mode, ip, dist, o))
    be.check(be.fn["debug_wicp_track"](C.byref(cfg), fptr(M_d), C.cast(cb, C.c_void_p), None, (C.c_float * 16)()), "debug_wicp_track")
    res["evaluations_per_track"] = len(calls)
    be.check(be.fn["tracker_destroy"](h), "destroy")
    return res


def main(reps=200):
    be = T.hip_backend()
    oracle = T.oracle_backend()
    small = TrackerConfig()
    small.noHierarchyLevels = WC.LEVELS; small.trackingRegime[:WC.LEVELS] = WC.REGIME
    small.distThresh = WC.DIST_THRESH; small.terminationThreshold = WC.TERMINATION
    out = {"tool": "wicp_tracker_bench", "sizes": [one_size(be, oracle, WC.SCENES["offaxis"], small, reps),
                                                   one_size(be, oracle, WC.SCENE_VGA, TrackerConfig.default(), reps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
