#!/usr/bin/env python3
"""Mesh smoothing timings on mesh_s_rgb_yaw (320x240, ITMVoxel_s_rgb, 5 mm, three fused frames; tests/mesh_attr_cases.py: 819 k
triangles, 405 k unique vertices): host microseconds, launch to stream idle, of itm_mesh_smooth
  * with steps = 0: the adjacency build and the topology pass (and the call's one wait),
  * with steps = 1 and steps = 21, in the gather form and in the scatter form (ITM_DEBUG_MESH_SMOOTH_SCATTER): one pass = the
    difference / 20, which leaves out everything a call does once,
  * with the default configuration (20 passes), both forms,
beside the bytes one pass must move and the wall time of the numpy restatement (tests/mesh_smooth_terms.py) on the same host.
Every figure is given for `reps` repetitions of `inner` calls, so the run-to-run spread is in the output.  One JSON line.
Run on the GPU:  python tools/mesh_smooth_bench.py [--reps 5] [--inner 10] [--scene NAME] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

DEBUG_MESH_SMOOTH_SCATTER = 31      # include/itm_debug.h


def timed(be, call, reps, inner):
    """microseconds per call"""
    out = []
    for _ in range(3):
        call()
    be.sync()
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        be.sync()
        out.append(round((time.perf_counter() - t0) / inner * 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--scene", default="mesh_s_rgb_yaw")
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import itm_testlib as T
    import mesh_attr_cases as MC
    import mesh_smooth_terms as MS
    be = T.hip_backend()
    sc = MC.SCENES[args.scene]
    ses = MC.fuse(be, sc, fused=True)
    m = capi.Mesh(ses.scene)
    m.MeshScene(); m.Index()
    vertices, faces = m.vertices(), m.faces()
    stats = m.Smooth(steps=0)
    n, _, _ = MS.topology(faces, len(vertices))
    entries = int(n.sum())
    res = {"library": be.version(), "scene": args.scene, "reps": args.reps, "inner": args.inner, "triangles": len(faces), "stats": stats, "entries": entries,
           # one gather pass: the iterate read and written once (16 B each), two row bounds and a flag byte per vertex, the rows (4 B per
           # entry); the neighbour gathers (16 B per entry) are served by the caches where the rows are local
           "pass_bytes_streamed": len(vertices) * (16 + 16 + 4 + 1) + entries * 4, "pass_bytes_gathered": entries * 16,
           "adjacency_us": timed(be, lambda: m.Smooth(steps=0), args.reps, args.inner)}
    for form, key in (("gather", 0), ("scatter", 1)):
        be.check(be.fn["debug_set"](DEBUG_MESH_SMOOTH_SCATTER, key), "debug_set")
        try:
            one = timed(be, lambda: m.Smooth(steps=1), args.reps, args.inner)
            many = timed(be, lambda: m.Smooth(steps=21), args.reps, args.inner)
            res[form] = {"steps_1_us": one, "steps_21_us": many, "pass_us": [round((b - a) / 20, 2) for a, b in zip(one, many)],
                         "default_call_us": timed(be, lambda: m.Smooth(), args.reps, args.inner)}
        finally:
            be.check(be.fn["debug_set"](DEBUG_MESH_SMOOTH_SCATTER, 0), "debug_set")
    if not args.no_numpy:
        t0 = time.perf_counter()
        MS.smooth(vertices, faces, MS.config(quantum=sc.voxelSize / 1024))
        res["numpy_default_call_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(res))
    m.close()
    ses.close()


if __name__ == "__main__":
    main()
