// Drives ITMMainEngine_HIP (include/itm_hip_engines.hpp) with TRACKER_WICP: per frame the weighted ICP tracker registers the depth
// image against the ICP maps of the previous frame, starting from the previous tracked pose, with weights from the view's sigmaZ
// image (computed although modelSensorNoise is off, as the reference's settings force it on); no pose comes from outside.  Prints
// one JSON line per frame with the tracked pose_d (column-major) and the microseconds of ProcessFrame; tests/test_wicp_engine.py
// compares the trajectory with the ground truth.
//   wicp_engine_demo <sequence file> <voxel / index: s | s_dense> [check frame]
// With a check frame k, frame k is also tracked through itm_tracker_weighted_track_camera on a handle of its own, from the same
// starting pose and maps, with a depth and sigmaZ image built here (the sigmaZ border cleared); the line of frame k then carries
// "same": whether the engine's pose equals it bit for bit.  Before the engine is created, device memory of the image's size is
// filled with 1.0f and freed, so that an engine that left its sigmaZ border uncleared would likely see weight-1 border pixels.
// sequence file: int32 {w, h, n}, float intr[4], int16 raw[n*h*w] (millimetres)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

template <class T> static bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

static void dirty_device_memory(size_t bytes) {
  std::vector<float> ones(bytes / 4, 1.0f);
  std::vector<void*> bufs(8, nullptr);
  for (void*& b : bufs) { check(itm_dev_malloc(&b, bytes), "malloc"); check(itm_memcpy_h2d(b, ones.data(), bytes, nullptr), "h2d"); }
  check(itm_stream_synchronize(nullptr), "sync");
  for (void* b : bufs) itm_dev_free(b);
}

template <class V, class I>
static int run(int w, int h, int n, const float* intr, const std::vector<int16_t>& raw, int checkFrame) {
  const size_t P = (size_t)w * h;
  dirty_device_memory(P * 4);
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_WICP;
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  calib.intrinsics_rgb.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  ITMSceneParams params(0.02f, 100, 0.005f, 0.2f, 3.0f, false);
  ITMMainEngine_HIP<V, I> engine(st, params, calib, Vector2i{w, h}, Vector2i{w, h});
  void *dRaw = nullptr, *dDepth = nullptr, *dScratch = nullptr, *dNormals = nullptr, *dSigma = nullptr;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc");
  check(itm_dev_malloc(&dDepth, P * 4), "malloc"); check(itm_dev_malloc(&dScratch, P * 4), "malloc");
  check(itm_dev_malloc(&dNormals, P * 16), "malloc"); check(itm_dev_malloc(&dSigma, P * 4), "malloc");
  itm_tracker* own = nullptr;
  check(itm_tracker_create(&own), "itm_tracker_create");
  itm_tracker_config cfg;
  std::memset(&cfg, 0, sizeof cfg);
  cfg.noHierarchyLevels = st.noHierarchyLevels;
  for (int i = 0; i < st.noHierarchyLevels && i < 8; ++i) cfg.trackingRegime[i] = st.trackingRegime[i];
  cfg.noICPRunTillLevel = st.noICPRunTillLevel; cfg.distThresh = st.depthTrackerICPThreshold; cfg.terminationThreshold = st.depthTrackerTerminationThreshold;
  for (int k = 0; k < n; ++k) {
    check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    float mine[16];
    const bool checking = k == checkFrame;
    if (checking) {
      std::vector<float> zeros(P, 0.0f);
      check(itm_memcpy_h2d(dSigma, zeros.data(), P * 4, nullptr), "h2d");
      check(itm_update_view((const int16_t*)dRaw, w, h, 1, 0.001f, 0.0f, calib.intrinsics_d.all, st.useBilateralFilter ? 1 : 0, 1, (float*)dDepth, (float*)dScratch,
                            (float*)dNormals, (float*)dSigma, nullptr), "update_view");
      ITMTrackingState* ts = engine.GetTrackingState();
      itm_view v;
      std::memset(&v, 0, sizeof v);
      v.depth = (const float*)dDepth; v.w = w; v.h = h;
      std::memcpy(v.M_d, ts->pose_d.GetM(), 64);
      std::memcpy(v.intr_d, calib.intrinsics_d.all, 16);
      check(itm_tracker_weighted_track_camera(own, &cfg, &v, (const float*)dSigma, ts->pointCloud_locations, ts->pointCloud_colours,
                                              ts->pose_pointCloud.GetM(), mine, nullptr), "weighted_track_camera");
    }
    const auto t0 = std::chrono::steady_clock::now();
    engine.ProcessFrame(nullptr, (const int16_t*)dRaw);
    check(itm_stream_synchronize(nullptr), "sync");
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    const float* M = engine.GetTrackingState()->pose_d.GetM();
    printf("{\"frame\": %d, \"us\": %.1f, ", k, us);
    if (checking) printf("\"same\": %s, ", std::memcmp(M, mine, 64) == 0 ? "true" : "false");
    printf("\"M\": [");
    for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", M[i]);
    printf("]}\n");
  }
  itm_tracker_destroy(own);
  for (void* p : {dRaw, dDepth, dScratch, dNormals, dSigma}) itm_dev_free(p);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s <sequence> <s|s_dense> [check frame]\n", argv[0]); return 2; }
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
  const int checkFrame = argc == 4 ? std::atoi(argv[3]) : -1;
  try {
    if (voxel == "s") return run<ITMVoxel_s, ITMVoxelBlockHash>(w, h, n, intr, raw, checkFrame);
    if (voxel == "s_dense") return run<ITMVoxel_s, ITMPlainVoxelArray>(w, h, n, intr, raw, checkFrame);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unknown voxel type %s\n", voxel.c_str());
  return 2;
}
