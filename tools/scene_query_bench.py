#!/usr/bin/env python3
"""Scene-query timings (itm_scene_query_points / itm_scene_cast_rays) on two scenes: `mesh_vga_4mm` (640x480, ITMVoxel_s, 4 mm, hash)
and BASELINE configs[4] (1280x960, ITMVoxel_f_rgb, 2 mm, hash pool 0x40000), three frames of the bench trajectory each.

  a  normal (+ colour where the voxel type has one) at the mesh's own vertices, beside itm_mesh_attributes through its
     one-lane-per-vertex kernel (ITM_DEBUG_MESH_ATTR_PER_VERTEX), which does the same reads: the yardstick of the kernel's quality
  b  the same outputs at as many points drawn uniformly from the bounding box of the allocated blocks: the incoherent case
  c  sdf only, for both point sets
  d  every camera ray of the last fused pose through itm_scene_cast_rays, beside FindSurface at that pose

Host microseconds per call, call to stream idle, inputs and outputs resident on the device: `--reps` repetitions of `--calls` calls
each (one synchronisation per repetition), median and range over the repetitions.  Kernel times: run this tool under
rocprofv3 --kernel-trace --stats -- python tools/scene_query_bench.py --reps 2, in a run of its own.  One JSON line.
Run on the GPU:  python tools/scene_query_bench.py [--reps 5] [--calls 20] [--scene vga|config4|both]"""
import argparse
import ctypes as C
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

DEBUG_MESH_ATTR_PER_VERTEX = 26
F = np.float32


def timed(be, reps, calls, fn):
    fn(); be.sync()                                     # warm-up: code objects, lazily allocated buffers
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        be.sync()
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def measure(be, sc, reps, calls):
    import itm_testlib as T
    import scene_query_terms as Q
    ses = T.Session(be, sc)
    for k in range(sc.frames):
        view = ses.frame(k, fused=True)
    scene = ses.scene
    mesh = capi.Mesh(scene)
    mesh.MeshScene()
    vertices = mesh.triangles().reshape(-1, 3)
    n = len(vertices)
    e = scene.download(capi.BUF_HASH_ENTRIES)
    pos = e["pos"][e["ptr"] >= 0].astype(np.int64)
    lo, hi = pos.min(0) * 8, (pos.max(0) + 1) * 8
    uniform = np.random.default_rng(1).uniform(lo, hi, (n, 3)).astype(F)
    res = {"vertices": int(n), "blocks": int(len(pos)), "voxel_type": capi.VOXEL_NAMES[sc.voxelType]}

    bufs = {"sdf": capi.DevBuffer(be, n * 4), "normal": capi.DevBuffer(be, n * 12), "colour": capi.DevBuffer(be, n * 4)}
    d_vertices, d_uniform = be.to_backend(vertices), be.to_backend(uniform)

    def query(points, units, names):
        out = capi.QueryOut()
        for w in names:
            setattr(out, w, bufs[w].ptr)
        return lambda: be.check(be.fn["scene_query_points"](capi._P(scene.h), capi._P(points.ptr), n, units, C.byref(out), None), "scene_query_points")

    attrs = ("normal", "colour") if sc.colour else ("normal",)
    what = capi.MESH_NORMALS | (capi.MESH_COLOURS if sc.colour else 0)
    res["a_query_vertices"] = timed(be, reps, calls, query(d_vertices, capi.QUERY_METRES, attrs))
    be.check(be.fn["debug_set"](DEBUG_MESH_ATTR_PER_VERTEX, 1), "debug_set")
    res["a_mesh_attributes_per_vertex"] = timed(be, reps, calls, lambda: mesh.ComputeAttributes(what))
    be.check(be.fn["debug_set"](DEBUG_MESH_ATTR_PER_VERTEX, 0), "debug_set")
    res["a_mesh_attributes_per_block"] = timed(be, reps, calls, lambda: mesh.ComputeAttributes(what))
    res["a_ratio_query_to_per_vertex"] = round(res["a_query_vertices"]["median_us"] / res["a_mesh_attributes_per_vertex"]["median_us"], 3)
    res["b_query_uniform"] = timed(be, reps, calls, query(d_uniform, capi.QUERY_VOXELS, attrs))
    res["c_sdf_vertices"] = timed(be, reps, calls, query(d_vertices, capi.QUERY_METRES, ("sdf",)))
    res["c_sdf_uniform"] = timed(be, reps, calls, query(d_uniform, capi.QUERY_VOXELS, ("sdf",)))

    # d: the camera rays of the last pose
    M, intr = view.M_d, sc.intr()
    scene.vis.CreateExpectedDepths(M, intr, ses.rs)
    rays = Q.camera_rays(M, intr, sc.w, sc.h, scene.download(capi.BUF_RANGE_IMAGE, ses.rs))
    d_rays, d_hits = be.to_backend(rays), capi.DevBuffer(be, len(rays) * 16)
    res["d_cast_rays"] = timed(be, reps, calls, lambda: be.check(be.fn["scene_cast_rays"](capi._P(scene.h), capi._P(d_rays.ptr), len(rays), capi._P(d_hits.ptr), None), "scene_cast_rays"))
    res["d_find_surface"] = timed(be, reps, calls, lambda: scene.vis.FindSurface(M, intr, ses.rs))
    res["d_ratio_cast_rays_to_find_surface"] = round(res["d_cast_rays"]["median_us"] / res["d_find_surface"]["median_us"], 3)
    hits = np.frombuffer(d_hits.numpy().tobytes(), F).reshape(-1, 4)
    surface = scene.download(capi.BUF_RAYCAST_RESULT, ses.rs).reshape(-1, 4)
    res["d_rays"] = int(len(rays))
    res["d_hits"] = int((hits[:, 3] > 0).sum())
    res["d_equal_to_find_surface"] = bool(np.array_equal(hits[:, 3], surface[:, 3]) and np.array_equal(hits[hits[:, 3] > 0], surface[surface[:, 3] > 0]))
    for b in list(bufs.values()) + [d_vertices, d_uniform, d_rays, d_hits]:
        b.close()
    mesh.close()
    ses.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--scene", default="both", choices=("vga", "config4", "both"))
    args = ap.parse_args()
    import itm_testlib as T
    import mesh_attr_cases as MC
    be = T.hip_backend()
    scenes = {"vga": MC.SCENES["mesh_vga_4mm"],
              "config4": T.Scenario(name="config4", w=1280, h=960, voxelType=T.VOXEL_F_RGB, voxelSize=0.002, mu=0.02, localBlockNum=0x40000, colour=True,
                                    trajectory="bench", frames=3)}
    res = {"library": be.version(), "reps": args.reps, "calls": args.calls}
    for name, sc in scenes.items():
        if args.scene in (name, "both"):
            res[name] = measure(be, sc, args.reps, args.calls)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
