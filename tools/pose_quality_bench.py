#!/usr/bin/env python3
"""Pose quality / tracking verdict timings (itm_pose_quality_*) at 640x480 on BASELINE configs[1]'s scene (hash TSDF, ITMVoxel_s, 4 mm
voxels, bench trajectory, 20 frames fused), for both wave shapes of the kernel (8 x 8 pixel tiles, the default; 64 consecutive pixels
of a row, ITM_DEBUG_POSE_QUALITY_ROWS).

  kernel        rocprofv3 --kernel-trace --stats around a child run of its own (--kernel-run): the kernel's device time per shape
  call          host clock around itm_pose_quality_evaluate (it returns with the counts on the host: that is its rendezvous), the two
                shapes alternated in blocks, at the true pose and at a pose 10 cm off along x
  closed loop   the frames/s of tools/closed_loop_bench.py's pipelined loop (update_view -> track_camera -> process_frame) with the verdict
                off and on (evaluate + verdict after the tracker; fuse only when GOOD, else expected depths + ICP maps alone), each in
                a child process, alternated; with --parent-lib also "off" on a build of the parent commit's library, to show that the
                loop without the verdict is what it was, within the spread of the repeats

One JSON line.  Run on the GPU:  python tools/pose_quality_bench.py [--reps 200] [--frames 100] [--repeats 3] [--parent-lib PATH] [--out FILE]"""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import infinitam_amd as itm  # noqa: E402
from infinitam_amd import capi, synth  # noqa: E402

W, H = 640, 480
FUSED, JUDGED = 20, 10


def stats(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def load(path=None):
    if not path:
        return itm.load()
    for fn in [n for n in capi._HOST_IO_SIGS if n.startswith("pose_quality_")]:      # a build of the parent commit has none of them
        capi._HOST_IO_SIGS.pop(fn)
    return capi.Backend(path, "itm_")


def fused_scene(be):
    intr = synth.intrinsics_for(W, H)
    scene = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.004), localBlockNum=0x40000)
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    pts = capi.DevBuffer(be, W * H * 16); nrm = capi.DevBuffer(be, W * H * 16)
    for k in range(FUSED):
        d = be.to_backend(synth.depth_frame(W, H, synth.bench_position(k), intr))
        scene.process_frame(capi.View(d, W, H, M_d=synth.pose_matrix(synth.bench_position(k)), intr_d=intr), rs, pts, nrm)
        be.sync()
        d.close()
    depth = be.to_backend(synth.depth_frame(W, H, synth.bench_position(JUDGED), intr))
    true = synth.pose_matrix(synth.bench_position(JUDGED))
    off = true.copy(); off[12] += np.float32(0.1)
    views = {"true": capi.View(depth, W, H, M_d=true, intr_d=intr), "x+10cm": capi.View(depth, W, H, M_d=off, intr_d=intr)}
    return scene, views


def set_rows(be, rows):
    be.check(be.fn["debug_set"](capi.DEBUG_POSE_QUALITY_ROWS, int(rows)), "debug_set")


def kernel_run(reps):
    """the child under rocprofv3: `reps` evaluations per shape and pose"""
    be = load()
    scene, views = fused_scene(be)
    q = capi.PoseQuality(be)
    for rows in (0, 1):
        set_rows(be, rows)
        for v in views.values():
            for _ in range(reps):
                q.evaluate(scene, v)
    set_rows(be, 0)
    q.close()


def kernel_times(reps):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "pq", "--", sys.executable, os.path.abspath(__file__), "--kernel-run", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed: " + r.stderr[-800:])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "pose_quality_kernel" not in row["Name"]:
                        continue
                    shape = "tiles" if row["Name"].split("<", 1)[1].split(">", 1)[0].replace(" ", "").endswith("true") else "rows"
                    out[shape] = {"kernel": row["Name"].split("(", 1)[0], "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3)}
        if set(out) != {"tiles", "rows"}:
            raise RuntimeError(f"kernel stats: found {sorted(out)}")
        return out


def call_times(reps):
    be = load()
    scene, views = fused_scene(be)
    q = capi.PoseQuality(be)
    cfg = capi.PoseQuality.default_config(be, scene.params.mu)
    res = {}
    for name, v in views.items():
        vs, out = v.struct(), capi.PoseQualityStats()
        us = {0: [], 1: []}
        counts = {}
        block = 25
        for b in range(2 * (reps // block) + 2):            # tiles, rows, tiles, rows ...; the first block of each warms up
            rows = b & 1
            set_rows(be, rows)
            for _ in range(block):
                t0 = time.perf_counter()
                rc = be.fn["pose_quality_evaluate"](capi._P(q.h), capi._P(scene.h), C.byref(vs), C.byref(cfg), C.byref(out), None, None)
                dt = (time.perf_counter() - t0) * 1e6
                be.check(rc, "pose_quality_evaluate")
                if b >= 2:
                    us[rows].append(dt)
            counts[rows] = out.as_dict()
        assert {k: counts[0][k] for k in ("noValid", "noKnown", "noInliers")} == {k: counts[1][k] for k in ("noValid", "noKnown", "noInliers")}
        res[name] = {"counts": counts[0], "verdict": capi.PoseQuality.verdict(be, out, cfg), "tiles_us": stats(us[0]), "rows_us": stats(us[1])}
    set_rows(be, 0)
    q.close()
    return res, be.version()


def loop_run(frames, verdict, lib):
    """the child of the closed-loop legs: tools/closed_loop_bench.py's pipelined loop, bilateral filter off"""
    be = load(lib)
    intr = synth.intrinsics_for(W, H)
    scene = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.004), localBlockNum=0x40000)
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    pts = capi.DevBuffer(be, W * H * 16); nrm = capi.DevBuffer(be, W * H * 16)
    raws = [be.to_backend(np.round(synth.depth_frame(W, H, synth.bench_position(k), intr) * 1000.0).astype(np.int16)) for k in range(frames)]
    depth = capi.DevBuffer(be, W * H * 4); scratch = capi.DevBuffer(be, W * H * 4)
    ip = (C.c_float * 4)(*intr)
    cfg = capi.TrackerConfig.default()
    view = capi.View(depth, W, H, M_d=synth.pose_matrix(synth.bench_position(0)), intr_d=intr).struct()
    out = (C.c_float * 16)()
    outp = C.cast(out, C.POINTER(C.c_float))
    Mview, Mout = np.ctypeslib.as_array(view.M_d), np.ctypeslib.as_array(out)
    Mp = C.cast(view.M_d, C.POINTER(C.c_float))
    if verdict:
        q = capi.PoseQuality(be)
        qcfg = capi.PoseQuality.default_config(be, scene.params.mu)
        qout, result = capi.PoseQualityStats(), C.c_int32()
    not_good = 0
    fps = []
    for rep in range(2):                                    # the first pass warms up
        scene.reco.ResetScene()
        Mview[:] = synth.pose_matrix(synth.bench_position(0)).astype(np.float32).reshape(16)
        be.sync(); t0 = None
        for k in range(frames):
            if k == 5:
                be.sync(); t0 = time.perf_counter()
            be.check(be.fn["update_view"](raws[k].ptr, W, H, 1, 0.001, 0.0, ip, 0, 0, depth.ptr, scratch.ptr, None, None, None), "update_view")
            good = True
            if k > 0:
                be.check(be.fn["track_camera"](C.byref(cfg), C.byref(view), pts.ptr, nrm.ptr, Mp, outp, None), "track")
                Mview[:] = Mout
                if verdict:
                    be.check(be.fn["pose_quality_evaluate"](capi._P(q.h), capi._P(scene.h), C.byref(view), C.byref(qcfg), C.byref(qout), None, None), "evaluate")
                    be.check(be.fn["pose_quality_verdict"](C.byref(qout), C.byref(qcfg), C.byref(result)), "verdict")
                    good = result.value == capi.TRACKING_GOOD
            if good:
                scene.process_frame(view, rs, pts, nrm)
            else:
                not_good += rep
                scene.vis.CreateExpectedDepths(Mview, intr, rs)
                be.check(be.fn["create_icp_maps"](capi._P(scene.h), C.byref(view), capi._P(rs.h), capi._P(pts.ptr), capi._P(nrm.ptr), None), "create_icp_maps")
        be.sync()
        fps.append((frames - 5) / (time.perf_counter() - t0))
    gt = synth.pose_matrix(synth.bench_position(frames - 1))
    print(json.dumps({"fps": round(fps[-1], 1), "not_good": not_good, "final_translation_error_m": round(float(np.abs(Mview[12:15] - gt[12:15]).max()), 5)}))


def closed_loop(frames, repeats, parent_lib):
    legs = [("off", 0, None), ("on", 1, None)] + ([("parent_off", 0, parent_lib)] if parent_lib else [])
    got = {name: [] for name, _, _ in legs}
    for _ in range(repeats):
        for name, verdict, lib in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--loop-run", "--frames", str(frames), "--verdict", str(verdict)] + (["--lib", lib] if lib else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"closed loop leg {name} failed: " + r.stderr[-800:])
            got[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {name: {"fps": stats([g["fps"] for g in v], 1), "runs": v} for name, v in got.items()}
    off, on = res["off"]["fps"]["median"], res["on"]["fps"]["median"]
    res["verdict_cost_us_per_frame"] = round(1e6 / on - 1e6 / off, 1)
    if parent_lib:
        res["off_over_parent_off"] = round(off / res["parent_off"]["fps"]["median"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--loop-run", action="store_true")
    ap.add_argument("--verdict", type=int, default=0)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.kernel_run:
        return kernel_run(args.reps)
    if args.loop_run:
        return loop_run(args.frames, bool(args.verdict), args.lib)
    # the children first: this process opens the GPU only afterwards
    kernels = kernel_times(max(args.reps // 4, 10))
    loop = closed_loop(args.frames, args.repeats, args.parent_lib)
    calls, version = call_times(args.reps)
    res = {"library": version, "image": [W, H], "scene": "BASELINE configs[1]: hash, ITMVoxel_s, 4 mm, bench trajectory, %d frames fused" % FUSED, "reps": args.reps,
           "kernel_us": kernels, "call_us": calls, "closed_loop": dict(loop, frames=args.frames, repeats=args.repeats)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
