#!/usr/bin/env python3
"""tests/golden/g_image_maps.{json,npz}: the reference's own IITMVisualisationEngine::DepthToUchar4 / WeightToUchar4 /
NormalToUchar4 (Engine/ITMVisualisationEngine.cpp:19-107) on the inputs of tests/image_map_cases.py.

A small driver written here is compiled in a temporary directory against the reference's sources where they lie; it wraps the
caller's arrays in the reference's image objects and calls the three static functions.  Only data is stored: per case the SHA-256
of the input and of the output, every 97th pixel of the output, the limits the map found (as float32 bit patterns) and the count of non-zero pixels.  Cases
whose values leave the range of the reference's float -> uchar cast are refused (image_map_cases.EXTRA_CASES are not run at all).
Run in the development container:  python tests/golden/make_golden_image_maps.py [reference-root]"""
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
import image_map_cases as IC  # noqa: E402
import image_map_terms as IT  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g_image_maps")

DRIVER = r'''
#include <cstring>
#include "ITMLib/Utils/ITMLibDefines.h"
#include "ITMLib/Engine/ITMVisualisationEngine.h"
using namespace ITMLib::Engine;

template <class T, class IMG> static IMG* wrap(const T* src, int w, int h) {
  IMG* img = new IMG(Vector2i(w, h), true, false);
  memcpy(img->GetData(MEMORYDEVICE_CPU), src, sizeof(T) * (size_t)w * h);
  return img;
}

// kind 0: DepthToUchar4, 1: WeightToUchar4, 2: NormalToUchar4.  dst is filled with 0xAB first: the functions clear it themselves.
extern "C" int ref_image_map(int kind, const float* src, unsigned char* dst, int w, int h) {
  ITMUChar4Image out(Vector2i(w, h), true, false);
  memset(out.GetData(MEMORYDEVICE_CPU), 0xAB, (size_t)w * h * 4);
  if (kind == 2) {
    ITMFloat4Image* in = wrap<Vector4f, ITMFloat4Image>((const Vector4f*)src, w, h);
    IITMVisualisationEngine::NormalToUchar4(&out, in);
    delete in;
  } else {
    ITMFloatImage* in = wrap<float, ITMFloatImage>(src, w, h);
    if (kind == 0) IITMVisualisationEngine::DepthToUchar4(&out, in); else IITMVisualisationEngine::WeightToUchar4(&out, in);
    delete in;
  }
  memcpy(dst, out.GetData(MEMORYDEVICE_CPU), (size_t)w * h * 4);
  return 0;
}
'''

KINDS = {"depth": 0, "weight": 1, "normal": 2}


def build(ref_root, tmp):
    src = os.path.join(tmp, "driver.cpp")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    so = os.path.join(tmp, "libimage_maps_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCOMPILE_WITHOUT_CUDA", "-fPIC", "-shared", "-w",
                    "-I" + ref_root, src, os.path.join(ref_root, "ITMLib", "Engine", "ITMVisualisationEngine.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.ref_image_map.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return lib


def reference_map(lib, kind, src):
    src = np.ascontiguousarray(src, np.float32)
    h, w = src.shape[:2]
    out = np.zeros((h, w, 4), np.uint8)
    assert lib.ref_image_map(KINDS[kind], src.ctypes.data, out.ctypes.data, w, h) == 0
    return out


def limits_of(kind, src):
    if kind == "depth":
        return [float(v) for v in IT.depth_limits(src)]
    if kind == "weight":
        return [float(IT.weight_limit(src))]
    return []


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/InfiniTAM"
    if not os.path.isdir(os.path.join(ref_root, "ITMLib")):
        raise SystemExit("reference sources not available")
    tmp = tempfile.mkdtemp()
    try:
        lib = build(ref_root, tmp)
        meta = {"generator": "reference IITMVisualisationEngine::DepthToUchar4 / WeightToUchar4 / NormalToUchar4, g++ -O2 -ffp-contract=off",
                "subset_stride": IC.SUBSET_STRIDE, "cases": {}}
        arrays = {}
        for name, (kind, src) in IC.GOLDEN_CASES.items():
            parts = {}
            IT.MAPS[kind](src, parts)
            if "values" in parts and not IT.in_conversion_range(parts["values"]):
                raise SystemExit(f"{name}: values outside the range of the reference's conversion; not a golden case")
            out = reference_map(lib, kind, src)
            meta["cases"][name] = {"kind": kind, "shape": list(src.shape), "input_sha256": IT.sha256(src), "output_sha256": IT.sha256(out),
                                   "limits_float32_bits": ["%08x" % np.float32(v).view(np.uint32) for v in limits_of(kind, src)], "nonzero_pixels": int(np.count_nonzero(out.reshape(-1, 4).any(axis=1)))}
            arrays[name] = out.reshape(-1, 4)[::IC.SUBSET_STRIDE]
            print(name, meta["cases"][name])
        with open(OUT + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        np.savez_compressed(OUT + ".npz", **arrays)
        print("npz bytes", os.path.getsize(OUT + ".npz"))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
