#!/usr/bin/env python3
"""Timings of the scene alignment (itm_scene_band_samples, itm_aligner_evaluate, itm_aligner_align) on one GPU, for
profiles/scene_align_notes.md.  Three inputs:

  corner64   the analytic room corner of tests/scene_align_terms.py (64^3 voxels of 1 cm as blocks of a hash scene, ITMVoxel_s): the
             band samples of the source frame's volume against the world frame's, from the 3 degree / 15 mm start
  vga4mm     the scene BASELINE configs[1] leaves after `--frames` frames (640x480, ITMVoxel_s, 4 mm, hash, bench trajectory): its own band
             samples against itself, from a start turned by 1 degree about the samples' centre and shifted by 5 mm
  vga4mm_s2  the same with stride 2

  band_samples   host microseconds of the call that fills the buffer (it synchronises the stream for the count)
  evaluate       host microseconds of one evaluation at the start pose: the call returns with the result (tagged records in pinned
                 memory), so this is launch + kernel + the record's way to the host
  align          host microseconds of the whole loop, its result and the error left over
  bytes          what an evaluation has to move at least: the samples (16 bytes each) and every DISTINCT voxel its valid and invalid
                 cells touch, two bytes each on the sdf-mirror path
  kernels        (--kernels) device time of every launch: a child run of this tool under rocprofv3 --kernel-trace --stats

Medians and spread over `--reps` repetitions after one that warms up.  One JSON line.
Run on the GPU:  python tools/scene_align_bench.py [--reps 15] [--frames 60] [--kernels]"""
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


def timed(be, call, reps):
    times, out = [], None
    for _ in range(reps + 1):                      # the first repetition warms up (code objects, records) and is dropped
        be.sync()
        t0 = time.perf_counter()
        out = call()
        be.sync()
        times.append(round((time.perf_counter() - t0) * 1e6, 1))
    times = times[1:]
    return {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times)}, out


def distinct_voxels(samples, M, voxel_size):
    """how many distinct voxels the cells of the samples touch at pose M"""
    x = samples[:, :3].astype(np.float64) @ np.asarray(M, np.float64)[:3, :3].T + np.asarray(M, np.float64)[:3, 3]
    i = np.floor(x / voxel_size).astype(np.int64) + (1 << 19)
    keys = []
    for k in range(8):
        keys.append(((i[:, 0] + (k & 1)) << 42) | ((i[:, 1] + ((k >> 1) & 1)) << 21) | (i[:, 2] + (k >> 2)))
    return int(len(np.unique(np.concatenate(keys))))


def measure(be, name, dst, src, init, truth, reps, **cfg_kw):
    import scene_align_terms as A
    cfg = dst.align_config(**cfg_kw)
    holder = {}

    def sample():
        if "buf" in holder:
            holder["buf"].close()
        holder["buf"], holder["count"] = src.band_samples(cfg)
    band, _ = timed(be, sample, min(reps, 5))
    buf, count = holder["buf"], holder["count"]
    aligner = capi.SceneAligner(be)
    aligner.set_samples(buf, count)
    ev_time, ev = timed(be, lambda: aligner.evaluate(dst, init, cfg), reps)
    al_time, (M, res) = timed(be, lambda: aligner.align(dst, init, cfg), reps)
    rot, trans = A.pose_error(M, truth)
    rot0, trans0 = A.pose_error(init, truth)
    host = buf.numpy() if count else np.zeros((0, 4), np.float32)
    voxels = distinct_voxels(host, init, float(dst.params.voxelSize))
    bytes_min = count * 16 + voxels * 2
    out = {"input": name, "samples": count, "band_samples": band, "evaluate": dict(ev_time, noValid=ev.noValid),
           "align": dict(al_time, status=capi.ALIGN_STATUS_NAMES[res.status], evaluations=res.evaluations, noValid=res.noValid, initialCost=res.initialCost,
                         finalCost=res.finalCost, conditioning=res.conditioning, start_error=[rot0, trans0], error=[rot, trans]),
           "bytes": {"samples": count * 16, "distinct_voxels": voxels, "least": bytes_min,
                     "GB_per_s_over_the_call": round(bytes_min / (ev_time["median_us"] * 1e-6) / 1e9, 2)}}
    aligner.close()
    buf.close()
    return out


def kernel_times(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "al", "--", sys.executable, os.path.abspath(__file__),
               "--reps", "3", "--frames", str(args.frames)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed: " + r.stderr[-800:])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if any(k in row["Name"] for k in ("align_eval", "band_")):
                        out[row["Name"].split("(", 1)[0]] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                                             "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    import mesh_dense_cases as MD
    import scene_align_terms as A
    be = T.hip_backend()
    res = {"library": be.version(), "reps": args.reps, "frames": args.frames, "inputs": []}

    # the analytic room corner
    scenes = []
    for voxels in A.analytic_pair(capi.VOXEL_S):
        s = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=A.VOXEL_SIZE, mu=A.MU), localBlockNum=0x1000)
        s.reco.ResetScene()
        table, blocks, _ = MD.dense_as_hash(voxels, (A.N,) * 3, (0, 0, 0), capi.VOXEL_S)
        s.upload(capi.BUF_HASH_ENTRIES, table)
        s.upload(capi.BUF_VOXEL_BLOCKS, blocks)
        scenes.append(s)
    res["inputs"].append(measure(be, "corner64", scenes[0], scenes[1], A.STARTS["3deg_15mm"], A.TRUTH, args.reps))
    for s in scenes:
        s.close()

    # the fused 640x480 scene of 4 mm voxels against itself
    sc = T.Scenario(name="align_bench", w=640, h=480, voxelSize=0.004, mu=0.02, localBlockNum=0x10000, trajectory="bench", frames=args.frames)
    ses = T.Session(be, sc)
    for k in range(args.frames):
        ses.frame(k, fused=True)
    probe, n = ses.scene.band_samples(ses.scene.align_config(stride=4))
    centre = probe.numpy()[:, :3].astype(np.float64).mean(0) if n else np.zeros(3)
    probe.close()
    shift = A.rigid(np.eye(3), centre)
    init = shift @ A.rigid(A.rotation((1, 1, 0), np.radians(1.0)), (0.003, -0.003, 0.0028)) @ np.linalg.inv(shift)
    res["inputs"].append(measure(be, "vga4mm", ses.scene, ses.scene, init, np.eye(4), args.reps))
    res["inputs"].append(measure(be, "vga4mm_s2", ses.scene, ses.scene, init, np.eye(4), args.reps, stride=2))
    ses.close()
    if args.kernels:
        res["kernels"] = kernel_times(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
