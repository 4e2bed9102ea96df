#!/usr/bin/env python3
"""tests/golden/g_wicp_tracker.{json,npz}: the weighted-ICP cases of tests/wicp_cases.py run on the REFERENCE's own
ITMWeightedICPTracker / ITMWeightedICPTracker_CPU / ITMLowLevelEngine_CPU / ITMPose.

The inputs -- ICP maps of three fused frames, the next depth frame and its sigmaZ image -- come from the reference's CPU engines
(oracle/_ref/libitm_ref.so: fusion, CreateICPMaps, ComputeNormalAndWeights); the oracle's CPU restatement must give the same bytes
(the tests regenerate the inputs with it).  A small driver written here and the reference translation units are compiled into a
shared library in a temporary directory that is removed afterwards.  Only data is stored: input digests, per-level digests of the
depth and weight pyramids, noValidPoints / f / nabla / hessian for every level and mode at fixed poses, TrackCamera from perturbed
starting poses and, for TRACE_STARTS, every evaluation TrackCamera made (level, mode, the inverse pose asked for, the sums returned).
Run in the development container:  python tests/golden/make_golden_wicp_tracker.py [reference-root]"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import itm_testlib as T  # noqa: E402
import wicp_cases as WC  # noqa: E402
from infinitam_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_wicp_tracker")
MAX_TRACE = 64

DRIVER = r'''
#include <cstring>
#include <cmath>
#include <vector>
#define private public
#define protected public
#include "ITMLib/Engine/ITMWeightedICPTracker.cpp"
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMWeightedICPTracker_CPU.cpp"
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMLowLevelEngine_CPU.h"
#include "ITMLib/Objects/ITMView.h"
#include "ITMLib/Objects/ITMTrackingState.h"
#include "ITMLib/Objects/ITMRGBDCalib.h"
#undef private
#undef protected
using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

static void set_m(Matrix4f& M, const float* m) { for (int i = 0; i < 16; ++i) M.m[i] = m[i]; }

// records every evaluation of TrackCamera: level, mode, the inverse pose, the sums
struct Probe : ITMWeightedICPTracker_CPU {
  float* trace = nullptr; int traceCap = 0, traceLen = 0;     // per record: level, mode, invPose[16], f, nabla[6], hessian[36], count
  Probe(Vector2i sz, TrackerIterationType* r, int levels, float dist, float term, const ITMLowLevelEngine* ll)
      : ITMWeightedICPTracker_CPU(sz, r, levels, 0, dist, term, ll) {}
  int ComputeGandH(float& f, float* nabla, float* hessian, Matrix4f approxInvPose) override {
    const int n = ITMWeightedICPTracker_CPU::ComputeGandH(f, nabla, hessian, approxInvPose);
    if (trace && traceLen < traceCap) {
      float* r = trace + 62 * traceLen++;
      r[0] = (float)levelId; r[1] = (float)iterationType;
      std::memcpy(r + 2, approxInvPose.m, 64); r[18] = f;
      // only the active block is written by ComputeGandH (3 or 6 parameters): the rest is recorded as 0
      const int np = iterationType == TRACKER_ITERATION_BOTH ? 6 : 3;
      for (int i = 0; i < 6; ++i) r[19 + i] = i < np ? nabla[i] : 0.0f;
      for (int c = 0; c < 6; ++c) for (int q = 0; q < 6; ++q) r[25 + q + 6 * c] = (q < np && c < np) ? hessian[q + 6 * c] : 0.0f;
      r[61] = (float)n;
    }
    return n;
  }
};

struct Inputs {
  ITMRGBDCalib calib; Vector2i sz; ITMView* view; ITMTrackingState* ts;
  Inputs(const float* depth, const float* sigma, int w, int h, const float* intr, const float* points, const float* normals, const float* scenePose)
      : sz(w, h) {
    calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    view = new ITMView(&calib, sz, sz, false);
    view->depthUncertainty = new ITMFloatImage(sz, true, false);
    std::memcpy(view->depth->GetData(MEMORYDEVICE_CPU), depth, (size_t)w * h * 4);
    std::memcpy(view->depthUncertainty->GetData(MEMORYDEVICE_CPU), sigma, (size_t)w * h * 4);
    ts = new ITMTrackingState(sz, MEMORYDEVICE_CPU);
    std::memcpy(ts->pointCloud->locations->GetData(MEMORYDEVICE_CPU), points, (size_t)w * h * 16);
    std::memcpy(ts->pointCloud->colours->GetData(MEMORYDEVICE_CPU), normals, (size_t)w * h * 16);
    Matrix4f S; set_m(S, scenePose); ts->pose_pointCloud->SetM(S);
  }
  ~Inputs() { delete ts; delete view; }
};

extern "C" {
// TrackCamera from M_d; trace (may be NULL): up to traceCap records of 62 floats; returns the number of evaluations
int ref_track(const float* depth, const float* sigma, int w, int h, const float* intr, const float* points, const float* normals,
              const float* scenePose, int levels, const int* regime, float dist, float term, const float* M_d, float* M_out,
              float* trace, int traceCap) {
  ITMLowLevelEngine_CPU ll;
  Inputs in(depth, sigma, w, h, intr, points, normals, scenePose);
  TrackerIterationType r[8];
  for (int i = 0; i < levels; ++i) r[i] = (TrackerIterationType)regime[i];
  Probe probe(in.sz, r, levels, dist, term, &ll);
  probe.trace = trace; probe.traceCap = traceCap;
  Matrix4f M; set_m(M, M_d); in.ts->pose_d->SetM(M);
  probe.TrackCamera(in.ts, in.view);
  std::memcpy(M_out, in.ts->pose_d->GetM().m, 64);
  return probe.traceLen;
}
// PrepareForEvaluation, then at each inverse pose, level and mode (1..3): out records of 62 floats as the trace's; the depth and
// weight pyramids into pyr (levels 1..levels-1 of each, consecutively: depth level 1, weight level 1, depth level 2, ...)
int ref_eval(const float* depth, const float* sigma, int w, int h, const float* intr, const float* points, const float* normals,
             const float* scenePose, int levels, float dist, int nInv, const float* invs, float* out, float* pyr) {
  ITMLowLevelEngine_CPU ll;
  Inputs in(depth, sigma, w, h, intr, points, normals, scenePose);
  TrackerIterationType r[8];
  for (int i = 0; i < levels; ++i) r[i] = TRACKER_ITERATION_BOTH;
  Probe probe(in.sz, r, levels, dist, 1e-3f, &ll);
  probe.SetEvaluationData(in.ts, in.view);
  probe.PrepareForEvaluation();
  for (int l = 1; l < levels; ++l) {
    ITMFloatImage* d = probe.viewHierarchy->levels[l]->depth; ITMFloatImage* g = probe.weightHierarchy->levels[l]->depth;
    std::memcpy(pyr, d->GetData(MEMORYDEVICE_CPU), d->dataSize * 4); pyr += d->dataSize;
    std::memcpy(pyr, g->GetData(MEMORYDEVICE_CPU), g->dataSize * 4); pyr += g->dataSize;
  }
  probe.trace = out; probe.traceCap = nInv * levels * 3;
  for (int k = 0; k < nInv; ++k)
    for (int l = 0; l < levels; ++l)
      for (int mode = 1; mode <= 3; ++mode) {
        probe.SetEvaluationParams(l);
        probe.iterationType = (TrackerIterationType)mode;
        Matrix4f inv; set_m(inv, invs + 16 * k);
        float f, nabla[6], hessian[36];
        std::memset(nabla, 0, sizeof nabla); std::memset(hessian, 0, sizeof hessian);
        probe.ComputeGandH(f, nabla, hessian, inv);
      }
  return probe.traceLen;
}
}
'''


def build(ref_root, tmp):
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    lib = os.path.join(ref_root, "ITMLib")
    units = [os.path.join(lib, "Engine", "DeviceSpecific", "CPU", "ITMLowLevelEngine_CPU.cpp"),
             os.path.join(lib, "Objects", "ITMPose.cpp")]
    so = os.path.join(tmp, "libwicp_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCOMPILE_WITHOUT_CUDA", "-fPIC", "-shared",
                    "-w", "-I" + ref_root, src] + units + ["-o", so], check=True)
    lib = C.CDLL(so)
    lib.ref_track.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_float, C.c_float] + \
        [C.c_void_p] * 3 + [C.c_int]
    lib.ref_eval.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 3
    return lib


def ptr(a):
    return a.ctypes.data


def unpack(records):
    """trace / evaluation records (62 floats) -> dict of arrays"""
    r = np.asarray(records, np.float32).reshape(-1, 62)
    return {"level": r[:, 0].astype(np.int32), "mode": r[:, 1].astype(np.int32), "inv": r[:, 2:18].copy(), "f": r[:, 18].copy(),
            "nabla": r[:, 19:25].copy(), "hessian": r[:, 25:61].copy(), "count": r[:, 61].astype(np.int32)}


def evaluate(lib, inputs, intr, levels, dist, invs):
    points, normals, M_d, depth, sigma = inputs
    h, w = depth.shape
    K = len(invs)
    out = np.zeros((K * levels * 3, 62), np.float32)
    sizes = [((w >> l), (h >> l)) for l in range(1, levels)]
    pyr = np.zeros(sum(2 * a * b for a, b in sizes) + 1, np.float32)
    invs = np.ascontiguousarray(invs, np.float32)
    n = lib.ref_eval(ptr(depth), ptr(sigma), w, h, ptr(intr), ptr(points), ptr(normals), ptr(M_d), levels, dist, K, ptr(invs), ptr(out), ptr(pyr))
    assert n == K * levels * 3
    levels_d, levels_w, o = [], [], 0
    for a, b in sizes:
        levels_d.append(pyr[o:o + a * b].reshape(b, a)); o += a * b
        levels_w.append(pyr[o:o + a * b].reshape(b, a)); o += a * b
    return unpack(out), levels_d, levels_w


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/InfiniTAM"
    if not os.path.isdir(os.path.join(ref_root, "ITMLib")):
        raise SystemExit("reference sources not available")
    ref = T.reference_backend()
    if ref is None:
        raise SystemExit("reference build not available (make -C oracle ref)")
    oracle = T.oracle_backend()
    tmp = tempfile.mkdtemp()
    try:
        lib = build(ref_root, tmp)
        meta = {"generator": "reference ITMWeightedICPTracker(_CPU) + ITMLowLevelEngine_CPU + ITMPose, g++ -O2 -ffp-contract=off; inputs from "
                             "the reference's CPU engines (" + ref.version() + ")",
                "levels": WC.LEVELS, "regime": WC.REGIME, "dist_thresh": WC.DIST_THRESH, "termination": WC.TERMINATION,
                "level_thresholds": WC.level_thresholds(), "scenes": {}}
        arrays = {}
        for name, sc in list(WC.SCENES.items()) + [("vga", WC.SCENE_VGA)]:
            inputs = WC.build(ref, sc)
            assert WC.digests(WC.build(oracle, sc)) == WC.digests(inputs), name      # the tests regenerate the inputs with the oracle
            points, normals, M_d, depth, sigma = inputs
            intr = np.array(sc.intr(), np.float32)
            invs = WC.eval_inv_poses(M_d)
            entry = {"inputs_sha256": WC.digests(inputs), "eval_order": list(invs.keys()), "eval_inv": [v.tolist() for v in invs.values()]}
            vga = name == "vga"
            levels = 1 if vga else WC.LEVELS
            thr = WC.level_thresholds()
            ev, pd, pw = evaluate(lib, inputs, intr, levels, np.float32(WC.DIST_THRESH), np.stack(list(invs.values())))
            # ref_eval evaluates every level with the threshold of ITS level (distThresh[levelId]): record them per record
            entry["eval_dist"] = [thr[l] if not vga else WC.DIST_THRESH for l in ev["level"]]
            entry["pyramid_sha256"] = {"depth": [synth.sha256(a) for a in pd], "weight": [synth.sha256(a) for a in pw]}
            np_d, np_w = WC.numpy_pyramid(depth, levels), WC.numpy_pyramid(sigma, levels)
            for l in range(1, levels):
                assert np.array_equal(np_d[l], pd[l - 1]) and np.array_equal(np_w[l], pw[l - 1]), (name, l)
            for k, v in ev.items():
                arrays[f"{name}_eval_{k}"] = v
            if not vga:
                tracks = {}
                for sname, M0 in WC.starts(M_d).items():
                    out = np.zeros(16, np.float32)
                    trace = np.zeros((MAX_TRACE, 62), np.float32)
                    n = lib.ref_track(ptr(depth), ptr(sigma), sc.w, sc.h, ptr(intr), ptr(points), ptr(normals), ptr(M_d), WC.LEVELS,
                                      ptr(np.array(WC.REGIME, np.int32)), WC.DIST_THRESH, WC.TERMINATION, ptr(M0), ptr(out),
                                      ptr(trace), MAX_TRACE)
                    assert 0 < n < MAX_TRACE
                    tracks[sname] = {"M_in": M0.tolist(), "M_out": out.tolist(), "evaluations": int(n)}
                    if sname in WC.TRACE_STARTS:
                        for k, v in unpack(trace[:n]).items():
                            arrays[f"{name}_trace_{sname}_{k}"] = v
                    print(name, sname, n, "evaluations", np.round(out[12:15], 6))
                entry["tracks"] = tracks
            meta["scenes"][name] = entry
        with open(OUT + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        np.savez_compressed(OUT + ".npz", **arrays)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
