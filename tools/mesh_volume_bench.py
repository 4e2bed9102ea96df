#!/usr/bin/env python3
"""Dense meshing timings on the dense 512^3 configuration (BASELINE configs[2]: ITMPlainVoxelArray 512^3, ITMVoxel_s, 4 mm, 640x480,
offset (-256, -256, 0)) after its standard frames: host microseconds, launch to stream idle, of itm_mesh_volume and of the buffer's
clear alone (itm_mesh_scene on a dense scene), each for `reps` repetitions of `inner` calls back to back, so the spread is in the
output.  One JSON line.  The three launches apart (mesh_bricks_kernel<VX, false> = count, mesh_brick_scan_kernel,
mesh_bricks_kernel<VX, true> = emit): run under  rocprofv3 --kernel-trace --stats --  ; the count pass's share of the 8 TB/s peak is
sx * sy * sz * sizeof(TVoxel) = `volume_bytes` over its kernel time.
Run on the GPU:  python tools/mesh_volume_bench.py [--reps 5] [--inner 20] [--frames 30] [--max-triangles N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import infinitam_amd as itm  # noqa: E402
from infinitam_amd import capi, synth  # noqa: E402



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
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--max-triangles", type=int, default=0)
    args = ap.parse_args()
    be = itm.load()
    W, H, vox, vs = 640, 480, capi.VOXEL_S, 0.004
    scene = be.create_scene(vox, capi.INDEX_DENSE, capi.default_params(voxelSize=vs, stopIntegratingAtMaxW=True))      # 512^3, offset (-256, -256, 0)
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    intr = synth.intrinsics_for(W, H)
    pts, nrm = capi.DevBuffer(be, W * H * 16), capi.DevBuffer(be, W * H * 16)
    for k in range(args.frames):
        t = synth.bench_position(k % 20)
        d = be.to_backend(synth.depth_frame(W, H, t, intr))
        scene.process_frame(capi.View(d, W, H, M_d=synth.pose_matrix(t), intr_d=intr), rs, pts, nrm)
    be.sync()
    m = capi.Mesh(scene, args.max_triangles)
    m.MeshVolume()
    n, cap = m.info()

    res = {"library": be.version(), "reps": args.reps, "inner": args.inner, "frames": args.frames, "triangles": n, "max_triangles": cap,
           "size": list(scene.cfg.denseSize)}
    res["mesh_scene_clear_us"] = timed(be, m.MeshScene, args.reps, args.inner)
    res["volume_all_us"] = timed(be, m.MeshVolume, args.reps, args.inner)
    res["volume_bytes"] = scene.cfg.denseSize[0] * scene.cfg.denseSize[1] * scene.cfg.denseSize[2] * be.fn["voxel_size_bytes"](vox)
    m.MeshVolume()
    assert m.info()[0] == n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
