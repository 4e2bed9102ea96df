#!/usr/bin/env python3
"""Distance-field timings (itm_scene_esdf / itm_esdf_transform) on the VGA 4 mm scene (`mesh_vga_4mm`: 640x480, ITMVoxel_s, hash, three
frames of the bench trajectory): a 256^3 box centred on the allocated blocks, surface sites, max_distance 0 (unbounded) and 64, the
lean call (dist2 and state) and the full one (nearest and distance too).

Device time between two hipEvents around `--calls` calls on the null stream, outputs resident on the device, after a warm-up call;
median and range over `--reps` repetitions.  The transform alone (itm_esdf_transform on the classification the scene call left) is
timed the same way; the classification's share is the difference.  Beside the times: the bytes the algorithm needs -- one voxel
read per cell plus the halo's face cells and a state byte written; per pass 4 bytes (8 with nearest) read and written per cell, the
x pass reading the state byte instead, the z pass reading it again and writing 4 bytes of distance where wanted.

Writes profiles/esdf_bench.json (and prints it).  Run on the GPU:  python tools/esdf_bench.py [--reps 7] [--calls 5] [--side 256]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402


class Events:
    """two hipEvents on the null stream of the runtime the library uses"""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            self.ok(self.rt.hipEventCreate(C.byref(e)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"hip runtime call failed ({rc})")

    def time_ms(self, fn, calls):
        self.ok(self.rt.hipEventRecord(self.a, None))
        for _ in range(calls):
            fn()
        self.ok(self.rt.hipEventRecord(self.b, None))
        self.ok(self.rt.hipEventSynchronize(self.b))
        ms = C.c_float()
        self.ok(self.rt.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return ms.value / calls


def timed(be, ev, reps, calls, fn):
    fn(); be.sync()                                     # warm-up: code objects
    out = [ev.time_ms(fn, calls) for _ in range(reps)]
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def algorithmic_bytes(origin, side, voxel_bytes, nearest, distance):
    cells = side ** 3
    tiles = 1
    for o in origin:
        tiles *= ((o + side - 1) >> 3) - (o >> 3) + 1
    per = 8 if nearest else 4
    return {"classification": tiles * 896 * voxel_bytes + cells,          # a tile and the face cells of its halo; the state byte
            "pass_x": cells * (1 + per), "pass_y": cells * 2 * per, "pass_z": cells * (2 * per + 1 + (4 if distance else 0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_bench.json"))
    args = ap.parse_args()
    import itm_testlib as T
    import mesh_attr_cases as MC
    be = T.hip_backend()
    ev = Events()
    sc = MC.SCENES["mesh_vga_4mm"]
    ses = T.Session(be, sc)
    for k in range(sc.frames):
        ses.frame(k, fused=True)
    scene = ses.scene
    e = scene.download(capi.BUF_HASH_ENTRIES)
    pos = e["pos"][e["ptr"] >= 0].astype(np.int64)
    lo, hi = pos.min(0) * 8, (pos.max(0) + 1) * 8
    side = args.side
    origin = [int(v) for v in (lo + hi) // 2 - side // 2]
    n = side ** 3
    box = capi.EsdfBox()
    box.origin[:] = origin
    box.size[:] = [side] * 3
    size = (C.c_int32 * 3)(side, side, side)
    bufs = {"dist2": capi.DevBuffer(be, n * 4, np.int32, (side,) * 3), "nearest": capi.DevBuffer(be, n * 4, np.int32, (side,) * 3),
            "distance": capi.DevBuffer(be, n * 4, np.float32, (side,) * 3), "state": capi.DevBuffer(be, n, np.uint8, (side,) * 3)}
    res = {"library": be.version(), "scene": "mesh_vga_4mm: 640x480, ITMVoxel_s, 4 mm, hash, 3 frames of the bench trajectory", "blocks": int(len(pos)),
           "box": {"origin": origin, "size": [side] * 3, "cells": n}, "sites": "surface", "min_weight": 1, "reps": args.reps, "calls": args.calls, "cases": {}}
    for R in (0, 64):
        for variant, names in (("lean", ("dist2", "state")), ("full", ("dist2", "nearest", "distance", "state"))):
            out = capi.EsdfOut()
            for w in names:
                setattr(out, w, bufs[w].ptr)
            whole = timed(be, ev, args.reps, args.calls, lambda: be.check(
                be.fn["scene_esdf"](capi._P(scene.h), C.byref(box), capi.ESDF_SITE_SURFACE, 1, R, C.byref(out), None), "scene_esdf"))
            passes = timed(be, ev, args.reps, args.calls, lambda: be.check(
                be.fn["esdf_transform"](capi._P(bufs["state"].ptr), size, R, float(sc.voxelSize), C.byref(out), None), "esdf_transform"))
            by = algorithmic_bytes(origin, side, scene.voxel_dtype.itemsize, "nearest" in names, "distance" in names)
            case = {"scene_esdf": whole, "esdf_transform": passes,
                    "classification_ms_by_difference": round(whole["median_ms"] - passes["median_ms"], 4), "algorithmic_bytes": by,
                    "transform_gb_per_s": round((by["pass_x"] + by["pass_y"] + by["pass_z"]) / (passes["median_ms"] * 1e-3) / 1e9, 1)}
            res["cases"][f"R{R}_{variant}"] = case
        state, dist2 = bufs["state"].numpy(), bufs["dist2"].numpy()
        res["cases"][f"R{R}_full"]["cells_site"] = int(np.count_nonzero(state & capi.ESDF_SITE))
        res["cases"][f"R{R}_full"]["cells_observed"] = int(np.count_nonzero(state & capi.ESDF_OBSERVED))
        res["cases"][f"R{R}_full"]["cells_none"] = int(np.count_nonzero(dist2 == capi.ESDF_NONE))
        res["cases"][f"R{R}_full"]["largest_dist2"] = int(dist2[dist2 != capi.ESDF_NONE].max())
    for b in bufs.values():
        b.close()
    ses.close()
    text = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
