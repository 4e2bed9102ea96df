// Drives ITMMainEngine_HIP (include/itm_hip_engines.hpp) with TRACKER_COLOR and useColourTracker = true: per frame the colour
// tracker aligns the rgb image with the point cloud Prepare rendered from the previous pose, the scene fuses depth and colour at
// the tracked pose, no pose comes from outside.  Prints one JSON line per frame with the tracked pose_d (column-major) and the
// microseconds of ProcessFrame; tests/test_colour_engine.py compares the trajectory with the ground truth.
//   colour_engine_demo <sequence file> <voxel: f_rgb | s_rgb>   closed loop
//   colour_engine_demo --colourless                             TRACKER_COLOR + useColourTracker on ITMVoxel_s: must be refused
// sequence file: int32 {w, h, n}, float intr[4], int16 raw[n*h*w] (millimetres), uint8 rgb[n*h*w*4]
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

static ITMLibSettings colour_settings() {
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_COLOR;
  st.useColourTracker = true;
  return st;
}

template <class V>
static int run(int w, int h, int n, const float* intr, const std::vector<int16_t>& raw, const std::vector<uint8_t>& rgb) {
  const size_t P = (size_t)w * h;
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  ITMSceneParams params(0.02f, 100, 0.005f, 0.2f, 3.0f, false);
  ITMMainEngine_HIP<V, ITMVoxelBlockHash> engine(colour_settings(), params, calib, Vector2i{w, h}, Vector2i{w, h});
  void *dRaw = nullptr, *dRgb = nullptr;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc"); check(itm_dev_malloc(&dRgb, P * 4), "malloc");
  for (int k = 0; k < n; ++k) {
    check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    check(itm_memcpy_h2d(dRgb, rgb.data() + (size_t)k * P * 4, P * 4, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    const auto t0 = std::chrono::steady_clock::now();
    engine.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    check(itm_stream_synchronize(nullptr), "sync");
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const float* M = engine.GetTrackingState()->pose_d.GetM();
    printf("{\"frame\": %d, \"us\": %.1f, \"M\": [", k, us);
    for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", M[i]);
    printf("]}\n");
  }
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--colourless") {
    try {
      ITMRGBDCalib calib;
      ITMSceneParams params(0.02f, 100, 0.005f, 0.2f, 3.0f, false);
      ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> engine(colour_settings(), params, calib, Vector2i{64, 48}, Vector2i{64, 48});
    } catch (const std::runtime_error& e) {
      printf("refused: %s\n", e.what());
      return 0;
    }
    printf("accepted\n");
    return 1;
  }
  if (argc != 3) { fprintf(stderr, "usage: %s <sequence> <f_rgb|s_rgb> | --colourless\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[3];
  float intr[4];
  if (!rd(f, hdr, 3) || !rd(f, intr, 4)) { fprintf(stderr, "short file\n"); return 2; }
  const int w = hdr[0], h = hdr[1], n = hdr[2];
  std::vector<int16_t> raw((size_t)n * w * h);
  std::vector<uint8_t> rgb((size_t)n * w * h * 4);
  if (!rd(f, raw.data(), raw.size()) || !rd(f, rgb.data(), rgb.size())) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);
  const std::string voxel = argv[2];
  try {
    if (voxel == "f_rgb") return run<ITMVoxel_f_rgb>(w, h, n, intr, raw, rgb);
    if (voxel == "s_rgb") return run<ITMVoxel_s_rgb>(w, h, n, intr, raw, rgb);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unknown voxel type %s\n", voxel.c_str());
  return 2;
}
