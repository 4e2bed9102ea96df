// Drives ITMMainEngine_HIP (include/itm_hip_engines.hpp) -- the reference's ITMMainEngine::ProcessFrame with its switches, its
// tracking controller and dense mapper (Engine/ITMMainEngine.cpp:111-127,194-197, ITMTrackingController.cpp:11-46,
// ITMDenseMapper.cpp:50-58) -- over a sequence of raw depth frames read from a file, and prints one JSON line per frame
// (age_pointCloud, requiresFullRendering, pose, digests of the tracking maps); tests/test_main_engine.py compares them with
// the same sequence run on the reference's objects.
//   main_engine_demo <sequence file>          parity run
//   main_engine_demo --bench <frames>         closed tracking + mapping loop on the 640x480 bench scene, frames/s
//   main_engine_demo --bench-host <frames>    the same with every raw frame arriving from page-locked host memory (ProcessFrameFromHost,
//                                             the next frame uploaded while the current one is tracked and fused)
//   main_engine_demo --bench-map[-host] <frames>   THIS FORK'S DEFAULT pipeline: TRACKER_EXTERNAL (Utils/ITMLibSettings.cpp:44) -- the pose source
//                                             writes pose_d before every frame (Engine/RosPoseSourceEngine.cpp:112-118), ITMMainEngine::ProcessFrame
//                                             builds the view from the raw frame, the tracker is a no-op, mapper + Prepare fuse and ray-cast
// sequence file: int32 {w, h, n, trackerType, useApproximateRaycast, skipPoints, flags}, float intr[4],
//                [flags & 2, a colour camera of its own: int32 {wc, hc, voxelType}, float voxelSize, float intrRgb[4], float rgbToDepth[16],
//                 float rgbToDepthInv[16]], int16 raw[n*h*w], float poses[n*16] (if flags & 1), uint8 fusion[n], uint8 mainProcessing[n],
//                [flags & 2: uint8 rgb[n*hc*wc*4], one colour image per frame]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s V;
typedef ITMVoxelBlockHash I;

static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
template <class T> static bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

static ITMLibSettings settings_for(int trackerType, bool approx, bool skip) {
  ITMLibSettings st;
  st.trackerType = trackerType == 0 ? ITMLibSettings::TRACKER_COLOR : trackerType == 1 ? ITMLibSettings::TRACKER_ICP : ITMLibSettings::TRACKER_EXTERNAL;
  st.useApproximateRaycast = approx; st.skipPoints = skip;
  return st;
}

static int bench(int frames, bool fromHost, bool externalPoses = false) {
  // the bench scene: sphere of radius 0.5 m at (0, 0, 1.5) in front of a wall at 2.5 m, triangle-wave trajectory
  const int W = 640, H = 480, P = W * H, distinct = 100;
  std::vector<int16_t> raw((size_t)distinct * P);
  auto tri = [](int k) { return std::abs(((k + 25) % 100) - 50) - 25; };
  for (int k = 0; k < distinct; ++k) {
    const float tx = 0.004f * (float)tri(k), ty = 0.002f * (float)tri(2 * k);
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
      const float dx = ((float)x - 320.f) / 580.f, dy = ((float)y - 240.f) / 580.f, ox = tx, oy = ty, oz = -1.5f;
      const float A = dx * dx + dy * dy + 1.f, B = 2.f * (ox * dx + oy * dy + oz), C = ox * ox + oy * oy + oz * oz - 0.25f, disc = B * B - 4.f * A * C;
      float z = 2.5f;
      if (disc > 0) { const float t = (-B - std::sqrt(disc)) / (2.f * A); if (t > 0) z = t; }
      raw[(size_t)k * P + y * W + x] = (int16_t)(z * 1000.f);
    }
  }
  void* dRaw; check(itm_dev_malloc(&dRaw, raw.size() * 2), "malloc");
  check(itm_memcpy_h2d(dRaw, raw.data(), raw.size() * 2, nullptr), "h2d");
  ITMLibSettings st = settings_for(externalPoses ? 2 : 1, false, true);
  ITMSceneParams params(0.02f, 100, 0.004f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  ITMMainEngine_HIP<V, I> engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x40000);
  void* hRaw = nullptr;
  if (fromHost) { check(itm_host_malloc(&hRaw, raw.size() * 2), "host malloc"); memcpy(hRaw, raw.data(), raw.size() * 2); }
  auto frame = [&](int k, bool more) {
    if (externalPoses) {      // the pose source of this fork: world -> camera for a camera at t, identity rotation
      float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      M[12] = -(0.004f * (float)tri(k)); M[13] = -(0.002f * (float)tri(2 * k));
      engine.GetTrackingState()->pose_d.SetM(M);
    }
    if (!fromHost) { engine.ProcessFrame(nullptr, (const int16_t*)dRaw + (size_t)(k % distinct) * P); return; }
    engine.ProcessFrameFromHost(nullptr, (const int16_t*)hRaw + (size_t)(k % distinct) * P, more ? (const int16_t*)hRaw + (size_t)((k + 1) % distinct) * P : nullptr);
  };
  for (int k = 0; k < 5; ++k) frame(k, true);
  check(itm_stream_synchronize(nullptr), "sync");
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 5; k < 5 + frames; ++k) frame(k, k + 1 < 5 + frames);
  check(itm_stream_synchronize(nullptr), "sync");
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const float* M = engine.GetTrackingState()->pose_d.GetM();
  const int last = 4 + frames;
  const float ex = -0.004f * (float)tri(last), ey = -0.002f * (float)tri(2 * last);
  printf("{\"frames\": %d, \"tracker\": \"%s\", \"raw_frames_from\": \"%s\", \"pose\": [%.9g, %.9g, %.9g], \"fps\": %.1f, \"ms_per_frame\": %.4f, \"final_translation_error_m\": %.5f}\n", frames, externalPoses ? "external poses (TRACKER_EXTERNAL, the fork's default): mapping only" : "ICP (closed loop)", fromHost ? "pinned host memory (stager)" : "device memory", M[12], M[13], M[14], frames / dt, 1e3 * dt / frames,
         std::fmax(std::fabs(M[12] - ex), std::fmax(std::fabs(M[13] - ey), std::fabs(M[14]))));
  itm_dev_free(dRaw);
  if (hRaw) itm_host_free(hRaw);
  return 0;
}

struct Sequence {
  int32_t hd[7]; float intr[4];
  int W = 0, H = 0, N = 0, Wc = 0, Hc = 0, voxelType = ITM_VOXEL_S;
  bool ownCamera = false;                    // the colour camera has its own size, intrinsics, pose and one image per frame
  float voxelSize = 0.005f, intrRgb[4], rgbToDepth[16], rgbToDepthInv[16];
  std::vector<int16_t> raw; std::vector<float> poses; std::vector<uint8_t> fusion, mainOn, rgb;
};

template <class TV>
static int parity(const Sequence& q) {
  const int W = q.W, H = q.H, N = q.N;
  const int32_t* hd = q.hd;
  const size_t P = (size_t)W * H, Pc = (size_t)q.Wc * q.Hc;
  ITMLibSettings st = settings_for(hd[3], hd[4] != 0, hd[5] != 0);
  ITMSceneParams params(0.02f, 100, q.voxelSize, 0.35f, 3.0f, false);      // ITMLibSettings.cpp:10
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(q.intr[0], q.intr[1], q.intr[2], q.intr[3]);
  calib.intrinsics_rgb.SetFrom(q.intrRgb[0], q.intrRgb[1], q.intrRgb[2], q.intrRgb[3]);
  if (q.ownCamera) { memcpy(calib.trafo_rgb_to_depth_calib, q.rgbToDepth, 64); memcpy(calib.trafo_rgb_to_depth_calib_inv, q.rgbToDepthInv, 64); }
  ITMMainEngine_HIP<TV, I> engine(st, params, calib, Vector2i{q.Wc, q.Hc}, Vector2i{W, H});
  const size_t PT = hd[3] == 0 ? Pc : P;      // the tracked image: the live render state and the point cloud have its size
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc"); check(itm_dev_malloc(&dRgb, Pc * 4), "malloc");
  std::vector<uint8_t> rgb(Pc * 4);
  for (size_t i = 0; i < Pc; ++i) { rgb[4 * i] = (uint8_t)(i % q.Wc); rgb[4 * i + 1] = (uint8_t)(i / q.Wc); rgb[4 * i + 2] = (uint8_t)((i % q.Wc) ^ (i / q.Wc)); rgb[4 * i + 3] = 255; }
  check(itm_memcpy_h2d(dRgb, rgb.data(), rgb.size(), nullptr), "h2d");
  std::vector<float> pts(PT * 4), col(PT * 4); std::vector<uint8_t> img(PT * 4); std::vector<int32_t> ids;
  for (int k = 0; k < N; ++k) {
    check(itm_memcpy_h2d(dRaw, q.raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    if (q.ownCamera) check(itm_memcpy_h2d(dRgb, q.rgb.data() + (size_t)k * Pc * 4, Pc * 4, nullptr), "h2d");
    ITMTrackingState* ts = engine.GetTrackingState();
    if (hd[6] & 1) ts->pose_d.SetM(q.poses.data() + 16 * k);            // the pose source of this fork writes it before the frame
    if (q.fusion[k]) engine.turnOnIntegration(); else engine.turnOffIntegration();
    if (q.mainOn[k]) engine.turnOnMainProcessing(); else engine.turnOffMainProcessing();
    engine.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    itm_counters c;
    check(itm_get_counters(engine.GetScene()->handle, engine.GetRenderState()->handle, &c, nullptr), "counters");
    const size_t nPts = hd[3] == 0 ? (size_t)c.noTotalPoints : P;
    check(itm_memcpy_d2h(pts.data(), ts->pointCloud_locations, nPts * 16, nullptr), "d2h");
    check(itm_memcpy_d2h(col.data(), ts->pointCloud_colours, nPts * 16, nullptr), "d2h");
    check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_RAYCAST_IMAGE, img.data(), img.size(), nullptr), "download");
    ids.resize((size_t)c.noVisibleEntries);
    if (c.noVisibleEntries) check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_VISIBLE_IDS, ids.data(), ids.size() * 4, nullptr), "download");
    const int32_t nv = c.noVisibleEntries;
    printf("{\"k\": %d, \"age\": %d, \"full\": %d, \"pose\": [", k, ts->age_pointCloud, ts->requiresFullRendering ? 1 : 0);
    for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", ts->pose_d.GetM()[i]);
    printf("], \"digest\": [\"%016llx\", \"%016llx\", \"%016llx\", \"%016llx\"], \"visible\": %d, \"points\": %zu}\n",
           (unsigned long long)fnv(pts.data(), nPts * 16), (unsigned long long)fnv(col.data(), nPts * 16), (unsigned long long)fnv(img.data(), img.size()),
           (unsigned long long)fnv(ids.data(), ids.size() * 4, fnv(&nv, 4)), nv, nPts);
  }
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "--bench")) return bench(atoi(argv[2]), false);
  if (argc >= 3 && !strcmp(argv[1], "--bench-host")) return bench(atoi(argv[2]), true);
  if (argc >= 3 && !strcmp(argv[1], "--bench-map")) return bench(atoi(argv[2]), false, true);
  if (argc >= 3 && !strcmp(argv[1], "--bench-map-host")) return bench(atoi(argv[2]), true, true);
  if (argc < 2) { fprintf(stderr, "usage: %s <sequence file> | --bench <frames>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Sequence q;
  if (!rd(f, q.hd, 7) || !rd(f, q.intr, 4)) return 2;
  q.W = q.hd[0]; q.H = q.hd[1]; q.N = q.hd[2]; q.Wc = q.W; q.Hc = q.H;
  memcpy(q.intrRgb, q.intr, 16);
  if (q.hd[6] & 2) {
    int32_t ext[3];
    if (!rd(f, ext, 3) || !rd(f, &q.voxelSize, 1) || !rd(f, q.intrRgb, 4) || !rd(f, q.rgbToDepth, 16) || !rd(f, q.rgbToDepthInv, 16)) return 2;
    q.Wc = ext[0]; q.Hc = ext[1]; q.voxelType = ext[2]; q.ownCamera = true;
  }
  const size_t P = (size_t)q.W * q.H, Pc = (size_t)q.Wc * q.Hc;
  q.raw.resize((size_t)q.N * P); q.poses.resize((size_t)q.N * 16); q.fusion.resize(q.N); q.mainOn.resize(q.N);
  if (!rd(f, q.raw.data(), q.raw.size()) || ((q.hd[6] & 1) && !rd(f, q.poses.data(), q.poses.size())) || !rd(f, q.fusion.data(), (size_t)q.N) || !rd(f, q.mainOn.data(), (size_t)q.N)) return 2;
  if (q.ownCamera) { q.rgb.resize((size_t)q.N * Pc * 4); if (!rd(f, q.rgb.data(), q.rgb.size())) return 2; }
  fclose(f);
  switch (q.voxelType) {
    case ITM_VOXEL_S: return parity<ITMVoxel_s>(q);
    case ITM_VOXEL_S_RGB: return parity<ITMVoxel_s_rgb>(q);
    case ITM_VOXEL_F_RGB: return parity<ITMVoxel_f_rgb>(q);
  }
  fprintf(stderr, "voxel type %d not built into this demo\n", q.voxelType);
  return 2;
}
