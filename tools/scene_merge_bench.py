#!/usr/bin/env python3
"""Scene-merge timings: two scenes of BASELINE configs[1] shape (640x480, ITMVoxel_s, 4 mm, hash; bench trajectory, streams 0 and 1,
`--frames` fused frames each, about 9 k blocks each) merged on one GPU by two routes:

  merge   itm_scene_merge into a FRESH copy of the first scene (the copy is restored by uploads between repetitions, outside the
          timed span): host microseconds from the call to stream idle, median and spread over `--reps` repetitions, with the
          statistics of the call (rounds, allocated, combined ...)
  host    what a library without the call offers: download both tables and pools, combine the blocks both scenes hold with numpy
          on the host, upload the pool again (the library then rebuilds the sdf mirror).  It allocates nothing, so it does LESS than
          the merge: blocks only the second scene holds are not brought over.

The combine phase moves (src read + dst read + dst write) x 512 voxels x 4 bytes per combined block; `combine_bytes` is that figure,
to be divided by the combine kernel's time.  Kernel times per phase (request, sweep, commit, list, combine): run this tool under
rocprofv3 --kernel-trace --stats -- python tools/scene_merge_bench.py --reps 3, in a run of its own.  One JSON line.
Run on the GPU:  python tools/scene_merge_bench.py [--reps 7] [--frames 220] [--no-host]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

POOL = 0x8000          # voxel blocks per scene: room for both scenes' blocks, 64 MB to restore per repetition
BUFS = (capi.BUF_HASH_ENTRIES, capi.BUF_EXCESS_LIST, capi.BUF_ALLOCATION_LIST, capi.BUF_VOXEL_BLOCKS)


def host_combine(src, dst, maxW):
    """CombineVoxelInformation for ITMVoxel_s on whole arrays (float32, the reference's operation order)."""
    f = np.float32
    oldW, newW = src["w_depth"].astype(np.int32), dst["w_depth"].astype(np.int32)
    on = oldW != 0
    sumW = oldW + newW
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (oldW.astype(f) * (src["sdf"].astype(f) / f(32767)) + newW.astype(f) * (dst["sdf"].astype(f) / f(32767))) / sumW.astype(f)
        enc = np.trunc(np.where(on, v, f(0)) * f(32767)).astype(np.int32).astype(np.int16)
    out = dst.copy()
    out["sdf"] = np.where(on, enc, dst["sdf"])
    out["w_depth"] = np.where(on, np.minimum(sumW, maxW), newW).astype(np.uint8)
    return out


def pos_keys(h):
    p = h["pos"].astype(np.int64) + 32768
    return (p[:, 0] << 32) | (p[:, 1] << 16) | p[:, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    be = T.hip_backend()
    mk = lambda stream: T.Scenario(name="merge_bench_%d" % stream, w=640, h=480, voxelSize=0.004, mu=0.02, localBlockNum=POOL, trajectory="bench",  # noqa: E731
                                   frames=args.frames, stream=stream)
    sessions = []
    for stream in (0, 1):
        ses = T.Session(be, mk(stream))
        for k in range(args.frames):
            ses.frame(k, fused=True)
        sessions.append(ses)
    a, b = sessions
    saved = [a.scene.download(w) for w in BUFS]
    ca = a.scene.counters()
    blocks = [POOL - 1 - s.scene.counters()["lastFreeBlockId"] for s in sessions]
    res = {"library": be.version(), "frames": args.frames, "reps": args.reps, "blocks": blocks}

    def restore():
        for w, arr in zip(BUFS, saved):
            a.scene.upload(w, arr)
        a.scene.set_counters(None, ca["lastFreeBlockId"], ca["lastFreeExcessListId"], 0)
        be.sync()

    times, stats = [], None
    for _ in range(args.reps + 1):                      # the first repetition warms up (scratch allocation, code objects) and is dropped
        restore()
        t0 = time.perf_counter()
        stats = a.scene.merge_from(b.scene)
        be.sync()
        times.append(round((time.perf_counter() - t0) * 1e6, 1))
    times = times[1:]
    res["merge"] = {"us": times, "median_us": statistics.median(times), "stats": stats, "combine_bytes": stats["combined"] * 512 * 4 * 3}

    if not args.no_host:
        restore()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            ha, hb = a.scene.download(capi.BUF_HASH_ENTRIES), b.scene.download(capi.BUF_HASH_ENTRIES)
            va, vb = a.scene.download(capi.BUF_VOXEL_BLOCKS).reshape(-1, 512), b.scene.download(capi.BUF_VOXEL_BLOCKS).reshape(-1, 512)
            la, lb = np.nonzero(ha["ptr"] >= 0)[0], np.nonzero(hb["ptr"] >= 0)[0]
            _, ia, ib = np.intersect1d(pos_keys(ha[la]), pos_keys(hb[lb]), return_indices=True)
            pa, pb = ha["ptr"][la[ia]], hb["ptr"][lb[ib]]
            va[pa] = host_combine(vb[pb], va[pa], int(a.scene.params.maxW))
            a.scene.upload(capi.BUF_VOXEL_BLOCKS, va.reshape(-1))
            be.sync()
            times.append(round((time.perf_counter() - t0) * 1e6, 1))
            restore()
        res["host"] = {"us": times, "median_us": statistics.median(times), "present_blocks": int(len(ia)), "pool_bytes_each_way": int(va.nbytes)}
    for s in sessions:
        s.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
