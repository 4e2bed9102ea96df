#!/usr/bin/env python3
"""The de-integration launch against the integration launch, same frame and same visible list, on the scenes of tools/config_bench.py:
  2: 640x480, ITMVoxel_s, 4 mm, hash (the bench.py workload; BASELINE configs[1])
  5: 1280x960, ITMVoxel_f_rgb, 2 mm, hash pool 0x40000 (BASELINE configs[4])
usage: python tools/deintegrate_bench.py [2|5] [rounds]      (development / measurement tool)
Fuses 30 frames, then alternates itm_integrate_into_scene and itm_deintegrate_from_scene (no statistics: nothing read back) of the last
frame `rounds` times -- the weights go W -> W + 1 -> W, so every round does the same work -- each call followed by a synchronise.
Prints one JSON line: the integration kernel's time by the library's event timers, and the host clock around each call + synchronise
(launch and synchronise overhead included, the same for both).  Kernel times proper: run it under `rocprofv3 --kernel-trace --stats`
and read integrate_hash_kernel / deintegrate_hash_kernel."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import infinitam_amd as itm  # noqa: E402
from infinitam_amd import capi, synth  # noqa: E402


def run(cfg: int, rounds: int):
    be = capi.Backend(os.environ['ITM_LIB'], 'itm_') if os.environ.get('ITM_LIB') else itm.load()
    if cfg == 5:
        W, H, vox, vs, colour = 1280, 960, capi.VOXEL_F_RGB, 0.002, True
    else:
        W, H, vox, vs, colour = 640, 480, capi.VOXEL_S, 0.004, False
    scene = be.create_scene(vox, capi.INDEX_HASH, capi.default_params(voxelSize=vs), localBlockNum=0x40000)
    scene.reco.ResetScene()
    rs = scene.vis.CreateRenderState((W, H))
    intr = synth.intrinsics_for(W, H)
    P = W * H
    pts, nrm = capi.DevBuffer(be, P * 16), capi.DevBuffer(be, P * 16)
    rgb = be.to_backend(synth.rgb_frame(W, H)) if colour else None
    frames = 30
    view = None
    for k in range(frames):
        t = synth.parity_position(k) if cfg == 5 else synth.bench_position(k)
        d = be.to_backend(synth.depth_frame(W, H, t, intr))
        view = capi.View(d, W, H, M_d=synth.pose_matrix(t), intr_d=intr, rgb=rgb, w_rgb=W, h_rgb=H, intr_rgb=intr)
        scene.process_frame(view, rs, pts, nrm)
    be.sync()
    for _ in range(3):                                # both kernels' code objects loaded, the frame's lines in cache for both
        scene.deintegrate(view, rs, keep_saturated=False)
        scene.reco.IntegrateIntoScene(view, rs)
    be.sync()
    scene.profile_read(reset=True)
    scene.profile_enable(1 << capi.TIMED_KERNELS.index("integrate"))
    t_int = t_de = 0.0
    for _ in range(rounds):
        t0 = time.perf_counter()
        scene.deintegrate(view, rs, keep_saturated=False)
        be.sync()
        t1 = time.perf_counter()
        scene.reco.IntegrateIntoScene(view, rs)
        be.sync()
        t2 = time.perf_counter()
        t_de += t1 - t0
        t_int += t2 - t1
    prof = scene.profile_read()["integrate"]
    t_stats = 0.0
    for _ in range(10):                               # the launch that counts, with its read-back
        t0 = time.perf_counter()
        st = scene.deintegrate(view, rs, keep_saturated=False, stats=True)
        t_stats += time.perf_counter() - t0
        scene.reco.IntegrateIntoScene(view, rs)
        be.sync()
    print(json.dumps({"config": cfg, "rounds": rounds, "visible_blocks": st["blocks"], "touched": st["touched"],
                      "integrate_kernel_us_event_timers": round(1e3 * prof["total_ms"] / max(1, prof["calls"]), 2),
                      "integrate_call_and_sync_us": round(1e6 * t_int / rounds, 2), "deintegrate_call_and_sync_us": round(1e6 * t_de / rounds, 2),
                      "deintegrate_with_stats_call_us": round(1e6 * t_stats / 10, 2)}))


if __name__ == "__main__":
    cfgs = [int(sys.argv[1])] if len(sys.argv) > 1 else [2, 5]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    for c in cfgs:
        run(c, n)
