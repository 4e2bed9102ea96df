#!/usr/bin/env python3
"""Mesh clean-up timings on two scenes -- mesh_vga_4mm (640x480, ITMVoxel_s, 4 mm; tests/mesh_attr_cases.py) and BASELINE configs[4]
(1280x960, ITMVoxel_f_rgb, 2 mm, 0x40000-block pool), three fused frames each: host microseconds, launch to stream idle, of
itm_mesh_index, itm_mesh_components (also with the per-lane statistics of ITM_DEBUG_MESH_COMPONENTS_PER_LANE) and
itm_mesh_filter_components (minTriangles = 100), with the counts (triangles, unique vertices, components, union rounds, what the filter
keeps).  The filter consumes its labelling, so every timed filter call follows an untimed re-mesh, re-index and re-label.
Every figure is given for `reps` repetitions of `inner` calls, so the run-to-run spread is in the output.  One JSON line.
Kernel times: run under rocprofv3 --kernel-trace --stats, in a run of its own.
Run on the GPU:  python tools/mesh_components_bench.py [--reps 5] [--inner 20] [--min-triangles 100] [--scene NAME]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

DEBUG_MESH_COMPONENTS_PER_LANE = 30      # include/itm_debug.h


def timed(be, call, reps, inner, prepare=None):
    """microseconds per call; `prepare` runs, untimed, before every call"""
    out = []
    for _ in range(3):
        if prepare:
            prepare()
        call()
    be.sync()
    for _ in range(reps):
        spent = 0.0
        if prepare is None:
            t0 = time.perf_counter()
            for _ in range(inner):
                call()
            be.sync()
            spent = time.perf_counter() - t0
        else:
            for _ in range(inner):
                prepare()
                be.sync()
                t0 = time.perf_counter()
                call()
                be.sync()
                spent += time.perf_counter() - t0
        out.append(round(spent / inner * 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--min-triangles", type=int, default=100)
    ap.add_argument("--scene", default=None)
    args = ap.parse_args()
    import itm_testlib as T
    import mesh_attr_cases as MC
    be = T.hip_backend()
    scenes = {"mesh_vga_4mm": MC.SCENES["mesh_vga_4mm"],
              "config4": T.Scenario(name="config4", w=1280, h=960, voxelType=T.VOXEL_F_RGB, voxelSize=0.002, localBlockNum=0x40000, colour=True,
                                    trajectory="bench", frames=3)}
    res = {"library": be.version(), "reps": args.reps, "inner": args.inner, "min_triangles": args.min_triangles, "scenes": {}}
    for name, sc in scenes.items():
        if args.scene and name != args.scene:
            continue
        ses = MC.fuse(be, sc, fused=True)
        m = capi.Mesh(ses.scene)

        def relabel():
            m.MeshScene(); m.Index(); m.Components()

        relabel()
        n, (nv, _), (nc, rounds) = m.info()[0], m.index_info(), m.components_info()
        sizes = sorted(m.components()["noTriangles"].tolist(), reverse=True)
        r = {"triangles": n, "unique_vertices": nv, "components": nc, "union_rounds": rounds, "largest_components": sizes[:3],
             "index_us": timed(be, m.Index, args.reps, args.inner),
             "components_us": timed(be, m.Components, args.reps, args.inner)}
        be.check(be.fn["debug_set"](DEBUG_MESH_COMPONENTS_PER_LANE, 1), "debug_set")
        try:
            r["components_per_lane_us"] = timed(be, m.Components, args.reps, args.inner)
        finally:
            be.check(be.fn["debug_set"](DEBUG_MESH_COMPONENTS_PER_LANE, 0), "debug_set")
        r["filter_us"] = timed(be, lambda: m.FilterComponents(args.min_triangles), args.reps, args.inner, prepare=relabel)
        relabel()
        r["kept_triangles"], r["kept_components"] = m.FilterComponents(args.min_triangles)
        res["scenes"][name] = r
        m.close()
        ses.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
