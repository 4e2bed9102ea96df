#!/usr/bin/env python3
"""Display-path timings (profiles/get_image.md): the three colour maps of infinitam_amd/csrc/image_maps.hip at 640x480 and 1280x960,
each beside a device-to-device copy that moves the same number of bytes in and out (the yardstick: a map is a stream of its input
and output plus one reduction pass over the input), and ITMMainEngine_HIP::GetImageDevice per image type after 20 frames of the
640x480 bench scene (BASELINE configs[1]; tests/cpp/get_image_demo.cpp --bench).

Map and copy times are device times between two stream events around `inner` back-to-back calls, after a warm-up, repeated `reps`
times: the median, the minimum and the maximum per call are reported.  Map and copy windows alternate, so both see the same machine.
One JSON line.  Launch counts and the absence of a host round trip: run under rocprofv3 --kernel-trace --stats (two kernels per depth /
weight map, one per normal map, no copy between them).
Run on the GPU:  python tools/get_image_bench.py [--reps 15] [--inner 200] [--calls 200] [--no-engine]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

SIZES = {"640x480": (640, 480), "1280x960": (1280, 960)}
# bytes per pixel read + written by the map's second launch / read by its first
TRAFFIC = {"depth": (4, 4, 4), "weight": (4, 4, 4), "normal": (16, 4, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    import torch
    import image_map_cases as IC
    import itm_testlib as T
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    be = T.hip_backend()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream

    def window(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(args.inner):
            call()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.inner

    def stats(v):
        return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}

    res = {"library": be.version(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "maps": {}}
    inputs = {"depth": IC.depth_image, "weight": IC.uncertainty_image, "normal": IC.normal_image}
    for tag, (w, h) in SIZES.items():
        for kind, (rd, wr, rd_limits) in TRAFFIC.items():
            src = torch.from_numpy(inputs[kind](w, h, 7)).cuda()
            dst = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            fn = be.fn[kind + "_to_uchar4"]
            # the yardstick: a copy that reads and writes (rd + wr) / 2 bytes per pixel -- the map's own stream of bytes
            half = w * h * (rd + wr) // 2
            ca, cb = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")

            def run_map():
                be.check(fn(src.data_ptr(), dst.data_ptr(), w, h, sp), kind)

            def run_copy():
                cb.copy_(ca, non_blocking=True)

            for _ in range(20):
                run_map(); run_copy()
            torch.cuda.synchronize()
            tm, tc = [], []
            for _ in range(args.reps):
                tm.append(window(run_map)); tc.append(window(run_copy))
            m, c = stats(tm), stats(tc)
            res["maps"][f"{kind}_{tag}"] = {"map": m, "copy_same_bytes": c, "map_over_copy": round(m["median_us"] / c["median_us"], 2),
                                            "bytes_streamed": w * h * (rd + wr), "bytes_reduction_pass": w * h * rd_limits}
    if not args.no_engine:
        import test_get_image as G
        r = subprocess.run([G.build_demo(), "--bench", str(args.calls)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        res["engine_640x480_configs1"] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
