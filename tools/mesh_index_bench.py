#!/usr/bin/env python3
"""Indexed-mesh timings on two scenes -- mesh_vga_4mm (640x480, ITMVoxel_s, 4 mm; tests/mesh_attr_cases.py) and BASELINE configs[4]
(1280x960, ITMVoxel_f_rgb, 2 mm, 0x40000-block pool), three fused frames each: host microseconds, launch to stream idle, of
itm_mesh_scene, itm_mesh_attributes (soup), itm_mesh_index and itm_mesh_indexed_attributes (normals, plus colours where the scene has
them), with the counts (triangles, soup vertices, unique vertices) and the sizes of the soup and the indexed PLY derived from them.
Every figure is given for `reps` repetitions of `inner` calls, so the run-to-run spread is in the output.  One JSON line.
--soup-only times itm_mesh_scene and itm_mesh_attributes alone and also loads a library built before the index existed
(ITM_LIB_OVERRIDE).  Kernel times: run under rocprofv3 --kernel-trace --stats, in a run of its own.
Run on the GPU:  python tools/mesh_index_bench.py [--reps 5] [--inner 20] [--soup-only] [--scene NAME]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi  # noqa: E402

INDEX_FNS = ("mesh_index", "mesh_index_info", "mesh_download_indexed", "mesh_indexed_attributes", "mesh_download_indexed_attributes",
             "mesh_write_ply_indexed", "mesh_write_obj_indexed")


def timed(be, call, reps, inner):
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
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--soup-only", action="store_true")
    ap.add_argument("--scene", default=None)
    args = ap.parse_args()
    if args.soup_only:
        for fn in INDEX_FNS:
            capi._HOST_IO_SIGS.pop(fn, None)
    import itm_testlib as T
    import mesh_attr_cases as MC
    be = T.hip_backend()
    scenes = {"mesh_vga_4mm": MC.SCENES["mesh_vga_4mm"],
              "config4": T.Scenario(name="config4", w=1280, h=960, voxelType=T.VOXEL_F_RGB, voxelSize=0.002, localBlockNum=0x40000, colour=True,
                                    trajectory="bench", frames=3)}
    res = {"library": be.version(), "reps": args.reps, "inner": args.inner, "scenes": {}}
    for name, sc in scenes.items():
        if args.scene and name != args.scene:
            continue
        ses = MC.fuse(be, sc, fused=True)
        m = capi.Mesh(ses.scene)
        m.MeshScene()
        what = capi.MESH_NORMALS | (capi.MESH_COLOURS if sc.colour else 0)
        n = m.info()[0]
        r = {"triangles": n, "mesh_scene_us": timed(be, m.MeshScene, args.reps, args.inner),
             "attributes_soup_us": timed(be, lambda: m.ComputeAttributes(what), args.reps, args.inner)}
        if not args.soup_only:
            m.Index()
            nv = m.index_info()[0]
            vb = 12 + 12 + (3 if sc.colour else 0)
            r.update({"soup_vertices": 3 * n, "unique_vertices": nv, "soup_ply_bytes": 3 * n * vb + 13 * n, "indexed_ply_bytes": nv * vb + 13 * n,
                      "index_us": timed(be, m.Index, args.reps, args.inner),
                      "attributes_indexed_us": timed(be, lambda: m.ComputeIndexedAttributes(what), args.reps, args.inner)})
        res["scenes"][name] = r
        m.close()
        ses.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
