#!/usr/bin/env python3
"""tests/golden/g_colour_tracker.{json,npz}: the colour-tracker cases of tests/colour_cases.py run on the REFERENCE's own
ITMColorTracker / ITMColorTracker_CPU / ITMLowLevelEngine_CPU / ITMPose.

The four reference translation units are compiled where they lie, together with a small driver written here (a subclass of
ITMColorTracker_CPU that exposes levelId / iterationType / F_oneLevel / G_oneLevel), into a shared library in a temporary
directory that is removed afterwards.  The driver zeroes the gradient images before the first PrepareForEvaluation: the reference
clears only the first three quarters of each (a Vector3s-sized memset per pixel of a Vector4s image) and never writes the border, so
the rest of its border holds whatever the allocation held (the hierarchy allocates every level at full size, and ChangeDims reallocates without clearing: seen non-zero garbage
on one level).  Only data is stored: input digests and the reference's outputs.
Run in the development container:  python tests/golden/make_golden_colour_tracker.py [reference-root]"""
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
import colour_cases as CC  # noqa: E402
from infinitam_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_colour_tracker")

DRIVER = r'''
#include <cstring>
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMColorTracker_CPU.h"
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMLowLevelEngine_CPU.h"
#include "ITMLib/Objects/ITMView.h"
#include "ITMLib/Objects/ITMTrackingState.h"
#include "ITMLib/Objects/ITMRGBDCalib.h"
using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

static void set_m(Matrix4f& M, const float* m) { for (int i = 0; i < 16; ++i) M.m[i] = m[i]; }

struct Probe : ITMColorTracker_CPU {
  Probe(Vector2i sz, TrackerIterationType* r, int L, const ITMLowLevelEngine* ll) : ITMColorTracker_CPU(sz, r, L, ll) {}
  void at(int level, TrackerIterationType it) { levelId = level; iterationType = it; }
  int valid() const { return countedPoints_valid; }
  ITMImageHierarchy<ITMViewHierarchyLevel>* hier() { return viewHierarchy; }
};

struct Setup {
  ITMLowLevelEngine_CPU ll;
  TrackerIterationType regime[8];
  ITMRGBDCalib calib;
  ITMView* view; ITMTrackingState* ts; Probe* probe;
  Setup(const unsigned char* rgb, int w, int h, const float* intr, int L, const int* reg, const float* calibM,
        const float* loc, const float* col, int n, const float* M_d) {
    for (int i = 0; i < L; ++i) regime[i] = (TrackerIterationType)reg[i];
    Vector2i sz(w, h);
    calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    Matrix4f cm; set_m(cm, calibM); calib.trafo_rgb_to_depth.SetFrom(cm);
    view = new ITMView(&calib, sz, sz, false);
    std::memcpy(view->rgb->GetData(MEMORYDEVICE_CPU), rgb, (size_t)w * h * 4);
    ts = new ITMTrackingState(sz, MEMORYDEVICE_CPU);
    std::memcpy(ts->pointCloud->locations->GetData(MEMORYDEVICE_CPU), loc, (size_t)n * 16);
    std::memcpy(ts->pointCloud->colours->GetData(MEMORYDEVICE_CPU), col, (size_t)n * 16);
    ts->pointCloud->noTotalPoints = n;
    Matrix4f M; set_m(M, M_d); ts->pose_d->SetM(M);
    probe = new Probe(sz, regime, L, &ll);
    // GradientX / Y write the interior only and memset 6 of the 8 bytes per pixel: the rest of the border is whatever the
    // allocation held.  Start from zeroed images of the final size (ChangeDims reallocates), the state the product's border rule
    // (0) restates.
    for (int l = 0; l < L; ++l) {
      ITMViewHierarchyLevel* lv = probe->hier()->levels[l];
      lv->gradientX_rgb->ChangeDims(Vector2i(w >> l, h >> l));
      lv->gradientY_rgb->ChangeDims(Vector2i(w >> l, h >> l));
      std::memset(lv->gradientX_rgb->GetData(MEMORYDEVICE_CPU), 0, lv->gradientX_rgb->dataSize * sizeof(Vector4s));
      std::memset(lv->gradientY_rgb->GetData(MEMORYDEVICE_CPU), 0, lv->gradientY_rgb->dataSize * sizeof(Vector4s));
    }
  }
  ~Setup() { delete probe; delete ts; delete view; }
};

extern "C" {
// TrackCamera; also returns calib_inv as the reference computes it
int ref_track(const unsigned char* rgb, int w, int h, const float* intr, int L, const int* reg, const float* calibM,
              const float* loc, const float* col, int n, const float* M_d, float* M_out, float* calibInv) {
  Setup s(rgb, w, h, intr, L, reg, calibM, loc, col, n, M_d);
  s.probe->TrackCamera(s.ts, s.view);
  std::memcpy(M_out, s.ts->pose_d->GetM().m, 64);
  std::memcpy(calibInv, s.calib.trafo_rgb_to_depth.calib_inv.m, 64);
  return 0;
}
// the pyramid of PrepareForEvaluation (through a TrackCamera on an empty cloud) and F / G at `pose` per level x type
int ref_eval(const unsigned char* rgb, int w, int h, const float* intr, int L, const float* loc, const float* col, int n,
             int nPoses, const float* poses, float* f, int* count, float* nabla, float* hessian,
             unsigned char* pyrRgb, short* pyrGx, short* pyrGy) {
  const int reg[8] = {3, 3, 3, 3, 3, 3, 3, 3};
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  Setup s(rgb, w, h, intr, L, reg, I, loc, col, n, I);
  s.ts->pointCloud->noTotalPoints = 0;
  s.probe->TrackCamera(s.ts, s.view);            // prepares the hierarchy; nothing to track
  s.ts->pointCloud->noTotalPoints = n;
  size_t off = 0;
  for (int l = 0; l < L; ++l) {
    ITMViewHierarchyLevel* lv = s.probe->hier()->levels[l];
    const size_t np = (size_t)lv->rgb->noDims.x * lv->rgb->noDims.y;
    std::memcpy(pyrRgb + 4 * off, lv->rgb->GetData(MEMORYDEVICE_CPU), np * 4);
    std::memcpy(pyrGx + 4 * off, lv->gradientX_rgb->GetData(MEMORYDEVICE_CPU), np * 8);
    std::memcpy(pyrGy + 4 * off, lv->gradientY_rgb->GetData(MEMORYDEVICE_CPU), np * 8);
    off += np;
  }
  int k = 0;
  for (int p = 0; p < nPoses; ++p)
    for (int l = 0; l < L; ++l)
      for (int t = 1; t <= 3; ++t, ++k) {
        Matrix4f M; set_m(M, poses + 16 * p);
        ITMPose pose(M);                        // SetM: the matrix as given, the parameters derived from it
        s.probe->at(l, (TrackerIterationType)t);
        s.probe->F_oneLevel(f + k, &pose);
        count[k] = s.probe->valid();
        s.probe->G_oneLevel(nabla + 6 * k, hessian + 36 * k, &pose);
      }
  return 0;
}
}
'''


def build(ref_root, tmp):
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    lib = os.path.join(ref_root, "ITMLib")
    units = [os.path.join(lib, "Engine", "ITMColorTracker.cpp"),
             os.path.join(lib, "Engine", "DeviceSpecific", "CPU", "ITMColorTracker_CPU.cpp"),
             os.path.join(lib, "Engine", "DeviceSpecific", "CPU", "ITMLowLevelEngine_CPU.cpp"),
             os.path.join(lib, "Objects", "ITMPose.cpp")]
    so = os.path.join(tmp, "libcolour_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCOMPILE_WITHOUT_CUDA", "-fPIC", "-shared",
                    "-w", "-I" + ref_root, src] + units + ["-o", so], check=True)
    return C.CDLL(so)


def fptr(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/InfiniTAM"
    if not os.path.isdir(os.path.join(ref_root, "ITMLib")):
        raise SystemExit("reference sources not available")
    tmp = tempfile.mkdtemp()
    try:
        so = build(ref_root, tmp)
        loc, col = CC.cloud()
        n = loc.shape[0]
        intr = np.array(CC.INTR, np.float32)
        meta = {"generator": "reference ITMColorTracker(_CPU) + ITMLowLevelEngine_CPU + ITMPose, g++ -O2 -ffp-contract=off",
                "cloud_sha256": [synth.sha256(loc), synth.sha256(col)], "n": n, "w": CC.W, "h": CC.H, "levels": CC.LEVELS}
        arrays = {}
        # pyramid + evaluations on the "both" frame, and the pyramid of an odd-sized frame
        M_both = CC.motions()["both"][0]
        for name, img, w, h, intr_i in (("vga", CC.frame(M_both), CC.W, CC.H, intr),
                                        ("odd", CC.odd_frame(), CC.ODD_W, CC.ODD_H, np.array(synth.intrinsics_for(CC.ODD_W, CC.ODD_H), np.float32))):
            img = np.ascontiguousarray(img)
            poses = np.stack(list(CC.eval_poses().values())).astype(np.float32)
            tot = sum((w >> l) * (h >> l) for l in range(CC.LEVELS))
            K = len(poses) * CC.LEVELS * 3
            f = np.zeros(K, np.float32); cnt = np.zeros(K, np.int32)
            nab = np.zeros((K, 6), np.float32); hes = np.zeros((K, 36), np.float32)
            pr = np.zeros(tot * 4, np.uint8); gx = np.zeros(tot * 4, np.int16); gy = np.zeros(tot * 4, np.int16)
            nn = n if name == "vga" else 0
            so.ref_eval(img.ctypes.data_as(C.c_void_p), w, h, fptr(intr_i), CC.LEVELS, fptr(loc), fptr(col), nn, len(poses), fptr(poses),
                        f.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), nab.ctypes.data_as(C.c_void_p),
                        hes.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), gx.ctypes.data_as(C.c_void_p),
                        gy.ctypes.data_as(C.c_void_p))
            meta[name + "_frame_sha256"] = synth.sha256(img)
            digests = []
            off = 0
            for lv in range(CC.LEVELS):
                m = (w >> lv) * (h >> lv)
                digests.append([synth.sha256(pr[4 * off:4 * (off + m)]), synth.sha256(gx[4 * off:4 * (off + m)]),
                                synth.sha256(gy[4 * off:4 * (off + m)])])
                off += m
            meta[name + "_pyramid_sha256"] = digests
            if name == "vga":
                arrays.update(eval_f=f, eval_count=cnt, eval_nabla=nab, eval_hessian=hes)
                meta["eval_order"] = "pose (identity, perturbed) x level 0..4 x type (ROTATION, TRANSLATION, BOTH)"
        # tracked poses
        tracks = {}
        cases = dict(CC.motions())
        for name, (M_true, calib, regime) in cases.items():
            img = np.ascontiguousarray(CC.frame(M_true, calib))
            calib = calib if calib is not None else CC.IDENTITY
            reg = np.array(regime or CC.REGIME, np.int32)
            out = np.zeros(16, np.float32); cinv = np.zeros(16, np.float32)
            so.ref_track(img.ctypes.data_as(C.c_void_p), CC.W, CC.H, fptr(intr), CC.LEVELS, reg.ctypes.data_as(C.c_void_p), fptr(calib),
                         fptr(loc), fptr(col), n, fptr(CC.IDENTITY), out.ctypes.data_as(C.c_void_p), cinv.ctypes.data_as(C.c_void_p))
            tracks[name] = {"frame_sha256": synth.sha256(img), "M_out": out.tolist(), "calib_inv": cinv.tolist()}
        # empty point cloud: f = MY_INF, zero gradient, the first step is below MIN_STEP; the pose comes back coerced
        img = np.ascontiguousarray(CC.frame(cases["t1cm"][0]))
        start = synth.pose_matrix_yaw((0.003, -0.001, 0.002), np.deg2rad(0.7))
        out = np.zeros(16, np.float32); cinv = np.zeros(16, np.float32)
        reg = np.array(CC.REGIME, np.int32)
        so.ref_track(img.ctypes.data_as(C.c_void_p), CC.W, CC.H, fptr(intr), CC.LEVELS, reg.ctypes.data_as(C.c_void_p), fptr(CC.IDENTITY),
                     fptr(loc), fptr(col), 0, fptr(start), out.ctypes.data_as(C.c_void_p), cinv.ctypes.data_as(C.c_void_p))
        tracks["empty"] = {"frame_sha256": synth.sha256(img), "M_in": np.asarray(start, np.float32).tolist(), "M_out": out.tolist()}
        meta["tracks"] = tracks
        with open(OUT + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        np.savez_compressed(OUT + ".npz", **arrays)
        for k, v in tracks.items():
            print(k, np.round(v["M_out"][12:15], 6))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
