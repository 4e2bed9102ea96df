// Asks a fused scene for its distance field through the C++ adapter: ITMMainEngine_HIP (poses from outside) fuses two raw depth
// frames of a corrugated wall, then ITMMainEngine_HIP::DistanceField transforms a box across the wall -- surface sites, distances
// bounded at 6 voxels -- and the scene is checkpointed into <dir>.
//   distance_field_demo <dir>
// Prints digests of the four outputs as JSON; tests/test_distance_field.py loads the checkpoint into a scene of its own, asks the
// Python binding the same question and compares.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;

static uint64_t fnv(const void* p, size_t bytes) {      // FNV-1a over the result bytes
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = (const uint8_t*)p;
  for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}

template <class T>
static std::vector<T> fetch(const void* dev, size_t n) {
  std::vector<T> v(n);
  check(itm_memcpy_d2h(v.data(), dev, n * sizeof(T), nullptr), "d2h");
  check(itm_stream_synchronize(nullptr), "sync");
  return v;
}

static int run(const char* dir) {
  const int W = 160, H = 120, P = W * H;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.f, 145.f, 80.f, 60.f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H});

  std::vector<int16_t> raw(P);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) raw[x + y * W] = (int16_t)(1500 + 2 * ((x * 7 + y * 13) % 50));      // millimetres
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  check(itm_memcpy_h2d(dRaw, raw.data(), (size_t)P * 2, nullptr), "h2d");
  for (int k = 0; k < 2; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.01f * k, 0, 0, 1};
    engine.GetTrackingState()->pose_d.SetM(M);
    engine.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
  }

  // a box across the wall (z = 1.5 .. 1.6 m at 1 cm voxels), its origin not block-aligned and left of / above the optical axis
  itm_esdf_box box = {{-21, -13, 143}, {40, 33, 17}};
  const size_t n = (size_t)box.size[0] * box.size[1] * box.size[2];
  void *dDist2, *dNearest, *dDistance, *dState;
  check(itm_dev_malloc(&dDist2, n * 4), "malloc"); check(itm_dev_malloc(&dNearest, n * 4), "malloc");
  check(itm_dev_malloc(&dDistance, n * 4), "malloc"); check(itm_dev_malloc(&dState, n), "malloc");
  itm_esdf_out out = {(int32_t*)dDist2, (int32_t*)dNearest, (float*)dDistance, (uint8_t*)dState};
  engine.DistanceField(box, out, ITM_ESDF_SITE_SURFACE, 1, 6);

  const std::vector<int32_t> dist2 = fetch<int32_t>(dDist2, n), nearest = fetch<int32_t>(dNearest, n);
  const std::vector<float> distance = fetch<float>(dDistance, n);
  const std::vector<uint8_t> state = fetch<uint8_t>(dState, n);
  uint32_t sites = 0, observed = 0, none = 0;
  for (size_t i = 0; i < n; ++i) {
    sites += (state[i] & ITM_ESDF_SITE) ? 1u : 0u;
    observed += (state[i] & ITM_ESDF_OBSERVED) ? 1u : 0u;
    none += dist2[i] == ITM_ESDF_NONE ? 1u : 0u;
  }
  check(itm_scene_save(engine.GetScene()->handle, nullptr, dir, nullptr), "scene_save");
  printf("{\"cells\": %zu, \"sites\": %u, \"observed\": %u, \"none\": %u, \"dist2\": \"%016llx\", \"nearest\": \"%016llx\", \"distance\": \"%016llx\", "
         "\"state\": \"%016llx\"}\n",
         n, sites, observed, none, (unsigned long long)fnv(dist2.data(), n * 4), (unsigned long long)fnv(nearest.data(), n * 4),
         (unsigned long long)fnv(distance.data(), n * 4), (unsigned long long)fnv(state.data(), n));
  for (void* p : {dRaw, dRgb, dDist2, dNearest, dDistance, dState}) itm_dev_free(p);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <checkpoint dir>\n", argv[0]); return 2; }
  try {
    return run(argv[1]);
  } catch (const std::exception& e) {
    fprintf(stderr, "distance_field_demo: %s\n", e.what());
    return 1;
  }
}
