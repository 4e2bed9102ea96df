#!/usr/bin/env python3
"""tests/golden/g_mesh_attributes.{json,npz}: the reference's own computeSingleNormalFromSDF and VoxelColorReader::interpolate
(DeviceAgnostic/ITMRepresentationAccess.h) at vertex / voxelSize for every vertex of the reference's mesh.

The scenes are fused and meshed by the reference's CPU engines (oracle/_ref/libitm_ref.so: ITMSceneReconstructionEngine_CPU,
ITMMeshingEngine_CPU); their hash table, voxel blocks and triangle buffer are handed to a small driver written here, compiled in a
temporary directory against the reference's headers where they lie, which calls the two functions per vertex.  Only data is
stored: SHA-256 digests of the full gradient and colour arrays and of the mesh, and the values for a subset of the vertices (every
k-th, plus the first 2 000 in buffer order whose sample position has a fractional part above 1 - 1e-3: floor(p) may sit one voxel
under the cell's corner there).  The oracle's CPU restatement must produce the same scene and mesh (the tests regenerate them with
it).  Run in the development container:  python tests/golden/make_golden_mesh_attributes.py [reference-root]"""
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
import mesh_attr_cases as MC  # noqa: E402
import mesh_attr_terms as MT  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_mesh_attributes")

DRIVER = r'''
#include "ITMLib/Utils/ITMLibDefines.h"
#include "ITMLib/Engine/DeviceAgnostic/ITMRepresentationAccess.h"
using namespace ITMLib::Objects;

template <class TVoxel>
static void run(const void* voxels, const void* table, const float* vertices, long n, float voxelSize, float* gradients, float* colours) {
  const TVoxel* data = (const TVoxel*)voxels;
  const ITMHashEntry* index = (const ITMHashEntry*)table;
  for (long i = 0; i < n; ++i) {
    const Vector3f p(vertices[3 * i] / voxelSize, vertices[3 * i + 1] / voxelSize, vertices[3 * i + 2] / voxelSize);
    const Vector3f g = computeSingleNormalFromSDF(data, index, p);
    gradients[3 * i] = g.x; gradients[3 * i + 1] = g.y; gradients[3 * i + 2] = g.z;
    if (colours) {
      const Vector4f c = VoxelColorReader<TVoxel::hasColorInformation, TVoxel, ITMVoxelBlockHash>::interpolate(data, index, p);
      colours[4 * i] = c.x; colours[4 * i + 1] = c.y; colours[4 * i + 2] = c.z; colours[4 * i + 3] = c.w;
    }
  }
}

extern "C" int ref_attributes(int voxelType, const void* voxels, const void* table, const float* vertices, long n, float voxelSize,
                              float* gradients, float* colours) {
  switch (voxelType) {
    case 0: run<ITMVoxel_s>(voxels, table, vertices, n, voxelSize, gradients, colours); return 0;
    case 1: run<ITMVoxel_f>(voxels, table, vertices, n, voxelSize, gradients, colours); return 0;
    case 2: run<ITMVoxel_s_rgb>(voxels, table, vertices, n, voxelSize, gradients, colours); return 0;
    case 3: run<ITMVoxel_f_rgb>(voxels, table, vertices, n, voxelSize, gradients, colours); return 0;
  }
  return -1;
}
extern "C" int ref_sizes(int* out) {
  out[0] = sizeof(ITMVoxel_s); out[1] = sizeof(ITMVoxel_f); out[2] = sizeof(ITMVoxel_s_rgb); out[3] = sizeof(ITMVoxel_f_rgb);
  out[4] = sizeof(ITMHashEntry); out[5] = SDF_BUCKET_NUM;
  return 0;
}
'''


def build(ref_root, tmp):
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    so = os.path.join(tmp, "libmesh_attr_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCOMPILE_WITHOUT_CUDA", "-fPIC", "-shared",
                    "-w", "-I" + ref_root, src, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.ref_attributes.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_void_p, C.c_void_p]
    lib.ref_sizes.argtypes = [C.c_void_p]
    return lib


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
        sizes = np.zeros(6, np.int32)
        lib.ref_sizes(sizes.ctypes.data)
        meta = {"generator": "reference computeSingleNormalFromSDF + VoxelColorReader::interpolate at vertex / voxelSize, g++ -O2 "
                             "-ffp-contract=off; scene and mesh from the reference's CPU engines (" + ref.version() + ")",
                "subset_halo": MT.SUBSET_HALO, "scenes": {}}
        arrays = {}
        for name, sc in MC.GOLDEN_SCENES.items():
            table, voxels, tri = MC.scene_and_mesh(ref, sc)
            t2, v2, tri2 = MC.scene_and_mesh(oracle, sc)
            assert np.array_equal(tri, tri2) and table.tobytes() == t2.tobytes(), name          # the tests regenerate them with the oracle
            for f in voxels.dtype.names:
                assert np.array_equal(voxels[f], v2[f]), (name, f)
            assert voxels.dtype.itemsize == sizes[sc.voxelType] and table.dtype.itemsize == sizes[4], "layout"
            assert (sc.bucketNum or int(sizes[5])) == int(sizes[5]), "the reference's functions are compiled for its SDF_BUCKET_NUM"
            vertices = np.ascontiguousarray(tri.reshape(-1, 3), np.float32)
            n = len(vertices)
            grad = np.zeros((n, 3), np.float32)
            col = np.zeros((n, 4), np.float32) if sc.colour else None
            voxels_c, table_c = np.ascontiguousarray(voxels), np.ascontiguousarray(table)
            rc = lib.ref_attributes(sc.voxelType, voxels_c.ctypes.data, table_c.ctypes.data, vertices.ctypes.data, n, np.float32(sc.voxelSize),
                                    grad.ctypes.data, col.ctypes.data if col is not None else None)
            assert rc == 0
            p = MT.sample_positions(vertices, sc.voxelSize)
            every, halo = MT.subset_indices(name, p)
            entry = {"vertices": n, "mesh_sha256": MT.sha256(tri), "gradient_sha256": MT.sha256(grad),
                     "high_fraction_1e-3": int(MT.high_fraction(p, 1e-3).sum()), "high_fraction_1e-5": int(MT.high_fraction(p, 1e-5).sum()),
                     "distinct_positions": int(len(np.unique(vertices.view(np.dtype((np.void, 12))).reshape(-1))))}
            arrays[f"{name}_every_gradient"] = grad[every]
            arrays[f"{name}_halo_index"] = halo.astype(np.int32)
            arrays[f"{name}_halo_gradient"] = grad[halo]
            if col is not None:
                entry["colour_sha256"] = MT.sha256(col)
                # the colour floats are multiples of small fractions; stored exactly as float32
                arrays[f"{name}_every_colour"] = col[every]
                arrays[f"{name}_halo_colour"] = col[halo]
            meta["scenes"][name] = entry
            print(name, entry)
        with open(OUT + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        np.savez_compressed(OUT + ".npz", **arrays)
        print("npz bytes", os.path.getsize(OUT + ".npz"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
