#!/usr/bin/env python3
"""Scene-prune timings: one scene of BASELINE configs[1] shape (640x480, ITMVoxel_s, 4 mm, hash with the default table of 1.18 M
slots; bench trajectory, `--frames` fused frames), pruned with empty and free-space blocks as candidates.

  dry    itm_scene_prune with dryRun (classify, candidates, chains, dropped ids, one count per render state): host microseconds from
         the call to its return (the call synchronises for the statistics), median and spread over `--reps` repetitions
  real   the same without dryRun on a FRESH copy of the scene (restored by uploads between repetitions, outside the timed span), with
         and without protection

`live_bytes` is what the classifying launch has to read of the pool: considered blocks x 512 voxels x 4 bytes (the table's 16 bytes per
slot come on top: `table_bytes`).  Kernel times per launch (prune_classify_kernel and the rest): run this tool under
rocprofv3 --kernel-trace --stats -- python tools/prune_bench.py --reps 5 --dry-only, in a run of its own.  One JSON line.
Run on the GPU:  python tools/prune_bench.py [--reps 9] [--frames 220] [--dry-only]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

POOL = 0x8000
BUFS = (capi.BUF_HASH_ENTRIES, capi.BUF_EXCESS_LIST, capi.BUF_ALLOCATION_LIST, capi.BUF_VOXEL_BLOCKS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--frames", type=int, default=220)
    ap.add_argument("--dry-only", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    be = T.hip_backend()
    sc = T.Scenario(name="prune_bench", w=640, h=480, voxelSize=0.004, mu=0.02, localBlockNum=POOL, trajectory="bench", frames=args.frames)
    ses = T.Session(be, sc)
    for k in range(args.frames):
        ses.frame(k, fused=True)
    scene, rs = ses.scene, ses.rs
    saved = [scene.download(w) for w in BUFS]
    ids, types = scene.download(capi.BUF_VISIBLE_IDS, rs), scene.download(capi.BUF_VISIBLE_TYPE, rs)
    c = scene.counters(rs)
    res = {"library": be.version(), "frames": args.frames, "reps": args.reps, "blocks": POOL - 1 - c["lastFreeBlockId"], "table_bytes": len(saved[0]) * 16}

    def restore():
        for w, arr in zip(BUFS, saved):
            scene.upload(w, arr)
        scene.upload(capi.BUF_VISIBLE_IDS, ids, rs); scene.upload(capi.BUF_VISIBLE_TYPE, types, rs)
        scene.set_counters(rs, c["lastFreeBlockId"], c["lastFreeExcessListId"], c["noVisibleEntries"])
        be.sync()

    def timed(cfg, fresh):
        times, stats = [], None
        for _ in range(args.reps + 1):                  # the first repetition warms up (scratch allocation, code objects) and is dropped
            if fresh:
                restore()
            t0 = time.perf_counter()
            stats = scene.prune(cfg)
            times.append(round((time.perf_counter() - t0) * 1e6, 1))
        times = times[1:]
        return {"us": times, "median_us": statistics.median(times), "stats": stats}

    res["dry"] = timed(scene.prune_config(dryRun=1), False)
    res["live_bytes"] = res["dry"]["stats"]["considered"] * 512 * 4
    if not args.dry_only:
        res["real_protected"] = timed(scene.prune_config(), True)
        res["real_unprotected"] = timed(scene.prune_config(protect=0), True)
    ses.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
