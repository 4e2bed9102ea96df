#!/usr/bin/env python3
"""Timings of the scene merge under a rigid transform (itm_scene_resample) on one GPU, for profiles/resample_notes.md.

  --scene bench   src is the scene BASELINE configs[1] leaves after its frames (640x480, ITMVoxel_s, 4 mm, hash; bench trajectory,
                  `--frames` fused frames), dst a freshly RESET scene of the same voxel size
  --scene test    the largest scenario of tests/test_scene_resample.py: scenario A (320x240, 1 cm) into a dst that holds scenario B
                  (rebuilt for every repetition; the build is outside the timed span)

  resample  the whole of src under a rotation of 0.3 rad about (1, 2, 3) with a fractional translation: host microseconds from the call
            to stream idle, median and spread over `--reps` repetitions after one that warms up, with the statistics of the call, the
            blocks of D, the candidates per participant and the share of the blocks of D in which no voxel of dst observed anything
            after the call into an EMPTY dst (the cost of the conservative candidate test)
  merge     itm_scene_merge of the same src into the same kind of dst, the same way
  kernels   (--kernels) the device time of every launch of both calls: a child run of this tool under rocprofv3 --kernel-trace --stats

ITM_TEST_LIB names another build of the library (the block kernel's two forms are builds with -DITM_RESAMPLE_STAGED=0 / 1).  One JSON line.
Run on the GPU:  python tools/resample_bench.py [--scene bench|test] [--reps 15] [--frames 220] [--kernels]"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

POOL = 0x10000         # voxel blocks per scene of the bench case (the candidates of 11 264 blocks need about 30 000)
# dstFromSrc: 0.3 rad about (1, 2, 3), translation (0.1234, -0.0567, 0.0891) m -- the transform of the tests
SKEW = np.array([0.958526731, 0.243323788, -0.148391441, 0, -0.230562791, 0.968097508, 0.0981226042, 0,
                 0.167532951, -0.0598395914, 0.984048724, 0, 0.123400003, -0.0566999987, 0.0891000032, 1], np.float32).reshape(4, 4).T


def timed(be, make_dst, call, reps):
    times, stats, dst = [], None, None
    for _ in range(reps + 1):                      # the first repetition warms up (scratch allocation, code objects) and is dropped
        dst = make_dst(dst)
        be.sync()
        t0 = time.perf_counter()
        stats = call(dst)
        be.sync()
        times.append(round((time.perf_counter() - t0) * 1e6, 1))
    times = times[1:]
    return {"us": times, "median_us": statistics.median(times), "min_us": min(times), "max_us": max(times), "stats": stats}, dst


def unobserved_share(dst):
    """Of the blocks dst holds, the share in which no voxel has a depth weight (dst was empty before the call)."""
    h = dst.download(capi.BUF_HASH_ENTRIES)
    w = dst.download(capi.BUF_VOXEL_BLOCKS)["w_depth"].reshape(-1, 512)
    ptr = h["ptr"][h["ptr"] >= 0]
    return round(float(np.count_nonzero(~w[ptr].any(axis=1))) / max(len(ptr), 1), 4), int(len(ptr))


def kernel_times(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "rs", "--", sys.executable, os.path.abspath(__file__),
               "--reps", "3", "--frames", str(args.frames), "--scene", args.scene]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed: " + r.stderr[-800:])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if any(k in row["Name"] for k in ("merge_", "resample_", "claim_blocks")):
                        out[row["Name"].split("(", 1)[0]] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("bench", "test"), default="bench")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    be = T.hip_backend()
    res = {"library": be.version(), "scene": args.scene, "reps": args.reps}
    if args.scene == "bench":
        sc = T.Scenario(name="resample_bench", w=640, h=480, voxelSize=0.004, mu=0.02, localBlockNum=POOL, trajectory="bench", frames=args.frames)
        src = T.Session(be, sc)
        for k in range(args.frames):
            src.frame(k, fused=True)
        res["frames"] = args.frames
        held = []

        def make_dst(old):
            if old is None:
                old = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.004, mu=0.02), localBlockNum=POOL)
                held.append(old)
            old.reco.ResetScene()
            return old
        empty_dst = make_dst
        size = 0.004
    else:
        import test_scene_merge as TM
        import test_scene_resample as TR
        src = TM.build(be, TR.fine_a())
        sessions = []

        def make_dst(old):
            for s in sessions:
                s.close()
            sessions[:] = [TM.build(be, TR.fine_b())]
            return sessions[0].scene

        def empty_dst(old):
            for s in sessions:
                s.close()
            sessions[:] = [T.Session(be, TR.fine_a())]
            return sessions[0].scene
        size = 0.01
    res["src_blocks"] = int(np.count_nonzero(src.scene.download(capi.BUF_HASH_ENTRIES)["ptr"] >= 0))
    q = capi.rigid_quantise(SKEW, size, be)
    if "scene_resample" in be.fn:
        r, dst = timed(be, make_dst, lambda d: d.resample_from(src.scene, q), args.reps)
        r["blocks_in_D"] = r["stats"]["resampled"] + r["stats"]["dstSwappedOut"]
        r["candidates_per_participant"] = round(r["stats"]["candidates"] / max(r["stats"]["considered"], 1), 2)
        d = empty_dst(dst if args.scene == "bench" else None)
        s = d.resample_from(src.scene, q)
        be.sync()
        share, blocks = unobserved_share(d)
        r["into_empty"] = {"stats": s, "blocks": blocks, "unobserved_share_of_D": share}
        res["resample"] = r
    r, dst = timed(be, make_dst, lambda d: d.merge_from(src.scene), args.reps)
    res["merge"] = r
    if args.kernels:
        res["kernels"] = kernel_times(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
