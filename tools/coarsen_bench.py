#!/usr/bin/env python3
"""Level-of-detail timings: the scene BASELINE configs[1] leaves after its frames (640x480, ITMVoxel_s, 4 mm, hash; bench trajectory,
`--frames` fused frames) resampled on one GPU.

  coarsen  itm_scene_coarsen into a freshly RESET scene of 8 mm voxels (the reset is outside the timed span): host microseconds from the
           call to stream idle, median and spread over `--reps` repetitions after one that warms up, with the statistics of the call
  merge    itm_scene_merge of the same src into a freshly reset scene of EQUAL voxel size, the same way: the same rounds over the same src
           table and the same src voxels read, only the voxel work differs.  With ITM_LIB_OVERRIDE naming a build of the parent commit
           and `--only merge` this is the figure "at the parent commit".
  kernels  (--kernels) the device time of every launch of both calls: a child run of this tool under rocprofv3 --kernel-trace --stats

`bytes` are what the voxel launch has to move, from the shapes: coarsen reads every participant's block once (the 27-block halo of a
coarse block re-reads its neighbours' faces: 17^3 / (2 * 8)^3 = 1.2 times that, counted) and writes `written` blocks plus their mirror
values; merge reads src and dst blocks and writes dst blocks.  One JSON line.
Run on the GPU:  python tools/coarsen_bench.py [--reps 15] [--frames 220] [--only coarsen|merge] [--kernels]"""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

POOL = 0x8000          # voxel blocks per scene
HBM_PEAK = 8.0e12      # bytes per second (MI355X data sheet)


def timed(be, dst, call, reps):
    times, stats = [], None
    for _ in range(reps + 1):                      # the first repetition warms up (scratch allocation, code objects) and is dropped
        dst.reco.ResetScene()
        be.sync()
        t0 = time.perf_counter()
        stats = call()
        be.sync()
        times.append(round((time.perf_counter() - t0) * 1e6, 1))
    times = times[1:]
    return {"us": times, "median_us": statistics.median(times), "min_us": min(times), "max_us": max(times), "stats": stats}


def kernel_times(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "lod", "--", sys.executable, os.path.abspath(__file__),
               "--reps", "3", "--frames", str(args.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed: " + r.stderr[-800:])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "merge_" in row["Name"] or "coarsen_" in row["Name"]:
                        out[row["Name"].split("(", 1)[0]] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--only", choices=("coarsen", "merge"))
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    be = T.hip_backend()
    sc = T.Scenario(name="coarsen_bench", w=640, h=480, voxelSize=0.004, mu=0.02, localBlockNum=POOL, trajectory="bench", frames=args.frames)
    src = T.Session(be, sc)
    for k in range(args.frames):
        src.frame(k, fused=True)
    blocks = POOL - 1 - src.scene.counters()["lastFreeBlockId"]
    res = {"library": be.version(), "frames": args.frames, "reps": args.reps, "src_blocks": blocks}
    vb = 512 * 4                                   # bytes of a voxel block of ITMVoxel_s
    if args.only != "merge" and "scene_coarsen" in be.fn:
        dst = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.008, mu=0.02), localBlockNum=POOL)
        r = timed(be, dst, lambda: dst.coarsen_from(src.scene), args.reps)
        w = r["stats"]["written"]
        r["bytes"] = {"read": int(w * 17 ** 3 * 4), "written": int(w * (vb + 512 * 2))}
        res["coarsen"] = r
        dst.close()
    if args.only != "coarsen":
        dst = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.004, mu=0.02), localBlockNum=POOL)
        r = timed(be, dst, lambda: dst.merge_from(src.scene), args.reps)
        c = r["stats"]["combined"]
        r["bytes"] = {"read": int(c * 2 * vb), "written": int(c * (vb + 512 * 2))}
        res["merge"] = r
        dst.close()
    src.close()
    if args.kernels:
        res["kernels"] = kernel_times(args)
        for call, kernel in (("coarsen", "coarsen_block_kernel"), ("merge", "merge_combine_kernel")):
            t = [v["average_us"] for k, v in res["kernels"].items() if kernel in k]
            if t and call in res:
                b = res[call]["bytes"]
                res[call]["voxel_launch"] = {"average_us": t[0], "bytes_per_s": round((b["read"] + b["written"]) / (t[0] * 1e-6)),
                                             "fraction_of_hbm_peak": round((b["read"] + b["written"]) / (t[0] * 1e-6) / HBM_PEAK, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
