#!/usr/bin/env python3
"""tests/golden/g_ren_tracker.{json,npz}: the Ren-tracker cases of tests/ren_cases.py run on the REFERENCE's own
ITMRenTracker / ITMRenTracker_CPU / ITMLowLevelEngine_CPU / ITMPose.

Each scene is fused from synth depth frames by the reference's CPU scene-reconstruction engine (oracle/_ref/libitm_ref.so, the
same build tests/golden/make_golden.py uses); its voxel blocks and hash table are copied into an ITMScene of a small driver
written here.  The driver and the reference translation units are compiled where they lie into a shared library in a temporary
directory that is removed afterwards; ITMRenTracker.cpp / ITMRenTracker_CPU.cpp are included by the driver so that the voxel /
index combinations under test can be instantiated.  Only data is stored: input digests (the depth frame, the fused voxels) and the
reference's outputs -- unprojected points, F / G and the valid count at fixed poses, TrackCamera from perturbed starting poses,
GetMFromParam of a few steps.
Run in the development container:  python tests/golden/make_golden_ren_tracker.py [reference-root]"""
import ctypes as C
import hashlib
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
import ren_cases as RC  # noqa: E402
from infinitam_amd import capi, synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_ren_tracker")

DRIVER = r'''
#include <cstring>
#include "ITMLib/Engine/ITMRenTracker.cpp"
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMRenTracker_CPU.cpp"
#include "ITMLib/Engine/DeviceSpecific/CPU/ITMLowLevelEngine_CPU.h"
#include "ITMLib/Objects/ITMScene.h"
#include "ITMLib/Objects/ITMView.h"
#include "ITMLib/Objects/ITMTrackingState.h"
#include "ITMLib/Objects/ITMRGBDCalib.h"
using namespace ITMLib::Engine;
using namespace ITMLib::Objects;

template class ITMLib::Engine::ITMRenTracker<ITMVoxel_f_rgb, ITMVoxelBlockHash>;
template class ITMLib::Engine::ITMRenTracker_CPU<ITMVoxel_f_rgb, ITMVoxelBlockHash>;
template class ITMLib::Engine::ITMRenTracker<ITMVoxel_s, ITMPlainVoxelArray>;
template class ITMLib::Engine::ITMRenTracker_CPU<ITMVoxel_s, ITMPlainVoxelArray>;

static void set_m(Matrix4f& M, const float* m) { for (int i = 0; i < 16; ++i) M.m[i] = m[i]; }

template <class TVoxel, class TIndex>
struct Probe : ITMRenTracker_CPU<TVoxel, TIndex> {
  Probe(Vector2i sz, TrackerIterationType* r, const ITMLowLevelEngine* ll, const ITMScene<TVoxel, TIndex>* s)
      : ITMRenTracker_CPU<TVoxel, TIndex>(sz, r, 2, ll, s) {}
  ITMFloat4Image* points() { return this->viewHierarchy->levels[0]->depth; }
  void F(float* f, const Matrix4f& invM) { this->levelId = 0; this->F_oneLevel(f, invM); }
  void G(float* g, float* h, const Matrix4f& invM) { this->levelId = 0; this->G_oneLevel(g, h, invM); }
  int count(const Matrix4f& invM) {       // points for which computePerPixelJacobian succeeds (G_oneLevel's valid points)
    ITMFloat4Image* p = points();
    const Vector4f* pts = p->GetData(MEMORYDEVICE_CPU);
    const TVoxel* vb = this->scene->localVBA.GetVoxelBlocks();
    const typename TIndex::IndexData* idx = this->scene->index.getIndexData();
    const float oo = 1.0f / (float)this->scene->sceneParams->voxelSize;
    int n = 0;
    for (int i = 0; i < (int)p->dataSize; ++i) {
      if (pts[i].w == -1.0f) continue;
      float j[6];
      if (computePerPixelJacobian<TVoxel, TIndex>(j, pts[i], vb, idx, oo, invM)) ++n;
    }
    return n;
  }
};

struct Base { virtual ~Base() {} virtual int run(const float* depth, int w, int h, const float* intr, const float* M_d, int nInv,
  const float* invs, float* points, float* f, float* nabla, float* hessian, int* count, float* M_out) = 0; };

template <class TVoxel, class TIndex>
struct Case : Base {
  ITMSceneParams params;
  ITMScene<TVoxel, TIndex>* scene;
  Case(float voxelSize, float mu, int maxW, const void* voxels, size_t voxelBytes, const void* entries, size_t entryBytes,
       const int* dsize, const int* doff)
      : params(mu, maxW, voxelSize, 0.35f, 3.0f, false) {
    scene = new ITMScene<TVoxel, TIndex>(&params, false, MEMORYDEVICE_CPU);
    set_index(scene->index, dsize, doff, entries, entryBytes);
    std::memcpy(scene->localVBA.GetVoxelBlocks(), voxels, voxelBytes);
  }
  static void set_index(ITMVoxelBlockHash& i, const int*, const int*, const void* e, size_t b) { std::memcpy(i.GetEntries(), e, b); }
  static void set_index(ITMPlainVoxelArray& i, const int* s, const int* o, const void*, size_t) {
    ITMPlainVoxelArray::IndexData* d = const_cast<ITMPlainVoxelArray::IndexData*>(i.getIndexData());
    d->size = Vector3i(s[0], s[1], s[2]); d->offset = Vector3i(o[0], o[1], o[2]);
  }
  ~Case() { delete scene; }
  int run(const float* depth, int w, int h, const float* intr, const float* M_d, int nInv, const float* invs, float* points,
          float* f, float* nabla, float* hessian, int* count, float* M_out) override {
    ITMLowLevelEngine_CPU ll;
    TrackerIterationType regime[2] = {TRACKER_ITERATION_BOTH, TRACKER_ITERATION_BOTH};
    ITMRGBDCalib calib;
    Vector2i sz(w, h);
    calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3], (float)w, (float)h);
    ITMView view(&calib, sz, sz, false);
    std::memcpy(view.depth->GetData(MEMORYDEVICE_CPU), depth, (size_t)w * h * 4);
    ITMTrackingState ts(sz, MEMORYDEVICE_CPU);
    Probe<TVoxel, TIndex> probe(sz, regime, &ll, scene);
    Matrix4f M; set_m(M, M_d); ts.pose_d->SetM(M);
    probe.TrackCamera(&ts, &view);                 // prepares level 0 as well
    std::memcpy(M_out, ts.pose_d->GetM().m, 64);
    std::memcpy(points, probe.points()->GetData(MEMORYDEVICE_CPU), (size_t)w * h * 16);
    for (int k = 0; k < nInv; ++k) {
      Matrix4f inv; set_m(inv, invs + 16 * k);
      probe.F(f + k, inv);
      probe.G(nabla + 6 * k, hessian + 36 * k, inv);
      count[k] = probe.count(inv);
    }
    return 0;
  }
};

extern "C" {
void* ref_case(int voxelType, int indexType, float voxelSize, float mu, int maxW, const void* voxels, size_t voxelBytes,
               const void* entries, size_t entryBytes, const int* dsize, const int* doff) {
  if (voxelType == 0 && indexType == 0) return new Case<ITMVoxel_s, ITMVoxelBlockHash>(voxelSize, mu, maxW, voxels, voxelBytes, entries, entryBytes, dsize, doff);
  if (voxelType == 3 && indexType == 0) return new Case<ITMVoxel_f_rgb, ITMVoxelBlockHash>(voxelSize, mu, maxW, voxels, voxelBytes, entries, entryBytes, dsize, doff);
  if (voxelType == 0 && indexType == 1) return new Case<ITMVoxel_s, ITMPlainVoxelArray>(voxelSize, mu, maxW, voxels, voxelBytes, entries, entryBytes, dsize, doff);
  return 0;
}
void ref_case_free(void* c) { delete (Base*)c; }
// TrackCamera from M_d (the tracked pose into M_out, the level-0 points into `points`), then F / G / valid count at each invM
int ref_run(void* c, const float* depth, int w, int h, const float* intr, const float* M_d, int nInv, const float* invs, float* points,
            float* f, float* nabla, float* hessian, int* count, float* M_out) {
  return ((Base*)c)->run(depth, w, h, intr, M_d, nInv, invs, points, f, nabla, hessian, count, M_out);
}
void ref_mrp(const float* step, float* M) {
  float s[6]; std::memcpy(s, step, sizeof s);
  Matrix4f m; GetMFromParam(s, m); std::memcpy(M, m.m, 64);
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
    so = os.path.join(tmp, "libren_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCOMPILE_WITHOUT_CUDA", "-fPIC", "-shared",
                    "-w", "-I" + ref_root, src] + units + ["-o", so], check=True)
    return C.CDLL(so)


def voxel_digest(vox):
    """SHA-256 per field of the voxel array (padding bytes never count)."""
    return {n: hashlib.sha256(np.ascontiguousarray(vox[n]).tobytes()).hexdigest() for n in vox.dtype.names}


def fused(be, sc):
    """The scene of `sc` fused by backend `be`: (voxel array, hash entries or None)."""
    ses = T.Session(be, sc)
    try:
        for k in range(sc.frames):
            ses.frame(k)
        vox = ses.scene.download(T.BUF_VOXEL_BLOCKS)
        ent = ses.scene.download(T.BUF_HASH_ENTRIES) if ses.scene.is_hash else None
    finally:
        ses.close()
    return vox, ent


def fptr(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/InfiniTAM"
    if not os.path.isdir(os.path.join(ref_root, "ITMLib")):
        raise SystemExit("reference sources not available")
    ref = T.reference_backend()
    if ref is None:
        raise SystemExit("reference build not available (make -C oracle ref)")
    tmp = tempfile.mkdtemp()
    try:
        so = build(ref_root, tmp)
        so.ref_case.restype = C.c_void_p
        so.ref_case.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p]
        so.ref_case_free.argtypes = [C.c_void_p]
        so.ref_run.argtypes = [C.c_void_p] + [C.c_void_p] * 1 + [C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 7
        meta = {"generator": "reference ITMRenTracker(_CPU) + ITMLowLevelEngine_CPU + ITMPose, g++ -O2 -ffp-contract=off; scenes fused by "
                             "the reference's CPU engines (" + ref.version() + ")",
                "eval_order": list(RC.eval_inv_poses(RC.SCENES["hash_s"]).keys()), "scenes": {}}
        arrays = {}
        for name, sc in RC.SCENES.items():
            vox, ent = fused(ref, sc)
            dep = RC.depth(sc)
            invs = np.stack(list(RC.eval_inv_poses(sc).values())).astype(np.float32)
            K = len(invs)
            dsize = np.array(sc.denseSize, np.int32); doff = np.array(sc.denseOffset or (0, 0, 0), np.int32)
            case = so.ref_case(sc.voxelType, sc.indexType, sc.voxelSize, sc.mu, sc.maxW, vox.ctypes.data, vox.nbytes,
                               ent.ctypes.data if ent is not None else None, ent.nbytes if ent is not None else 0,
                               dsize.ctypes.data, doff.ctypes.data)
            assert case, name
            entry = {"voxel_sha256": voxel_digest(vox), "depth_sha256": synth.sha256(dep), "tracks": {}}
            intr = np.array(sc.intr(), np.float32)
            for sname, M_d in RC.starts().items():
                pts = np.zeros((sc.h, sc.w, 4), np.float32)
                f = np.zeros(K, np.float32); nab = np.zeros((K, 6), np.float32); hes = np.zeros((K, 36), np.float32)
                cnt = np.zeros(K, np.int32); out = np.zeros(16, np.float32)
                so.ref_run(case, dep.ctypes.data, sc.w, sc.h, intr.ctypes.data, np.ascontiguousarray(M_d, np.float32).ctypes.data, K,
                           invs.ctypes.data, pts.ctypes.data, f.ctypes.data, nab.ctypes.data, hes.ctypes.data, cnt.ctypes.data,
                           out.ctypes.data)
                entry["tracks"][sname] = {"M_in": np.asarray(M_d, np.float32).tolist(), "M_out": out.tolist()}
                print(name, sname, np.round(out[12:15], 6))
            so.ref_case_free(C.c_void_p(case))
            entry["points_sha256"] = synth.sha256(pts)
            arrays[name + "_f"] = f
            arrays[name + "_nabla"] = nab
            arrays[name + "_hessian"] = hes
            arrays[name + "_count"] = cnt
            entry["eval_inv"] = invs.tolist()
            meta["scenes"][name] = entry
        mrp = []
        for s in RC.MRP_STEPS:
            m = np.zeros(16, np.float32)
            so.ref_mrp(fptr(np.array(s, np.float32)), m.ctypes.data_as(C.POINTER(C.c_float)))
            mrp.append({"step": list(s), "M": m.tolist()})
        meta["mrp"] = mrp
        with open(OUT + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        np.savez_compressed(OUT + ".npz", **arrays)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
