// Drives ITMMainEngine_HIP (include/itm_hip_engines.hpp) with TRACKER_REN: per frame the Ren tracker registers the depth image
// against the TSDF the earlier frames fused, starting from the previous tracked pose; the scene fuses the frame at the tracked pose,
// no pose comes from outside.  Prints one JSON line per frame with the tracked pose_d (column-major) and the microseconds of
// ProcessFrame; tests/test_ren_engine.py compares the trajectory with the ground truth.
//   ren_engine_demo <sequence file> <voxel / index: s | f | s_dense>
// sequence file: int32 {w, h, n}, float intr[4], int16 raw[n*h*w] (millimetres)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

template <class T> static bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

template <class V, class I>
static int run(int w, int h, int n, const float* intr, const std::vector<int16_t>& raw) {
  const size_t P = (size_t)w * h;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_REN;
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  ITMSceneParams params(0.02f, 100, 0.005f, 0.2f, 3.0f, false);
  ITMMainEngine_HIP<V, I> engine(st, params, calib, Vector2i{w, h}, Vector2i{w, h});
  void* dRaw = nullptr;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc");
  for (int k = 0; k < n; ++k) {
    check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    engine.ProcessFrame(nullptr, (const int16_t*)dRaw);
    check(itm_stream_synchronize(nullptr), "sync");
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const float* M = engine.GetTrackingState()->pose_d.GetM();
    printf("{\"frame\": %d, \"us\": %.1f, \"M\": [", k, us);
    for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", M[i]);
    printf("]}\n");
  }
  itm_dev_free(dRaw);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <sequence> <s|f|s_dense>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[3];
  float intr[4];
  if (!rd(f, hdr, 3) || !rd(f, intr, 4)) { fprintf(stderr, "short file\n"); return 2; }
  const int w = hdr[0], h = hdr[1], n = hdr[2];
  std::vector<int16_t> raw((size_t)n * w * h);
  if (!rd(f, raw.data(), raw.size())) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);
  const std::string voxel = argv[2];
  try {
    if (voxel == "s") return run<ITMVoxel_s, ITMVoxelBlockHash>(w, h, n, intr, raw);
    if (voxel == "f") return run<ITMVoxel_f, ITMVoxelBlockHash>(w, h, n, intr, raw);
    if (voxel == "s_dense") return run<ITMVoxel_s, ITMPlainVoxelArray>(w, h, n, intr, raw);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unknown voxel type %s\n", voxel.c_str());
  return 2;
}
