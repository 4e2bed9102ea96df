#!/usr/bin/env python3
"""Keyframe relocaliser timings (itm_reloc_*) at 640x480 with the default settings (4 levels -> 40x30, radius-6 blur, 500 ferns of 4
decisions, rows of 512 bytes).

  process_frame   host clock around itm_reloc_process_frame (encode + search + harvest decision; the call ends in its one
                  synchronise), depth resident on the device, harvesting off, at each database size
  search          device events around the search's two launches (itm_debug_reloc_search_ms) at each database size; bytes = N x rowBytes,
                  and the share of the 8 TB/s HBM peak that rate is
  stream_copy     tools/microbench/stream_copy in the same run, when it has been built: the rate a plain copy reaches

Databases are random codes (numpy default_rng(1)); the search reads every row whatever it holds.  One JSON line.
Run on the GPU:  python tools/reloc_bench.py [--reps 200] [--sizes 1000,65536] [--out profiles/reloc_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from infinitam_amd import capi, synth  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def stats(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def stream_copy_rate():
    exe = os.path.join(ROOT, "tools", "microbench", "stream_copy")
    if not os.path.exists(exe):
        return None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return {"returncode": r.returncode, "output": r.stdout.strip().splitlines()[-3:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", default="1000,65536")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import itm_testlib as T
    be = T.hip_backend()
    w, h = 640, 480
    depth = be.to_backend(synth.depth_frame(w, h, synth.bench_position(0), synth.intrinsics_for(w, h)))
    r = capi.Relocaliser(be, w, h)
    F = int(r.cfg.numFerns)
    row_bytes = (F + 15) & ~15
    res = {"library": be.version(), "image": [w, h], "small_image": [r.small[1], r.small[0]], "ferns": F, "decisions": int(r.cfg.numDecisions),
           "row_bytes": row_bytes, "reps": args.reps, "sizes": {}}
    rng = np.random.default_rng(1)
    ms = C.c_float()
    for n in [int(x) for x in args.sizes.split(",")]:
        r.upload(rng.integers(0, 16, (n, F)).astype(np.uint8), np.zeros((n, 16), np.float32))
        be.check(be.fn["debug_reloc_search_ms"](capi._P(r.h), 1, None), "debug_reloc_search_ms")
        host_us, search_us = [], []
        for i in range(args.reps + 5):
            t0 = time.perf_counter()
            r.process_frame(depth, None, False, 0.2, 1)
            dt = (time.perf_counter() - t0) * 1e6
            be.check(be.fn["debug_reloc_search_ms"](capi._P(r.h), 1, C.byref(ms)), "debug_reloc_search_ms")
            if i >= 5:                                      # the first calls load code objects
                host_us.append(dt)
                search_us.append(ms.value * 1e3)
        be.check(be.fn["debug_reloc_search_ms"](capi._P(r.h), 0, None), "debug_reloc_search_ms")
        plain_us = []
        for i in range(args.reps):                          # the same call without the two event records
            t0 = time.perf_counter()
            r.process_frame(depth, None, False, 0.2, 1)
            plain_us.append((time.perf_counter() - t0) * 1e6)
        nbytes = n * row_bytes
        rate = nbytes / (statistics.median(search_us) * 1e-6)
        res["sizes"][str(n)] = {"rows": n, "bytes": nbytes, "process_frame_host_us": stats(plain_us), "process_frame_host_us_with_events": stats(host_us),
                                "search_device_us": stats(search_us, 3), "search_bytes_per_s": round(rate, 0),
                                "share_of_8TBps_peak": round(rate / PEAK_BYTES_PER_S, 4)}
    res["stream_copy"] = stream_copy_rate()
    r.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
