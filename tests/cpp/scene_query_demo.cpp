// Asks a fused scene questions through the C++ adapter: two frames of a corrugated wall with a colour pattern are fused into an
// ITMVoxel_s_rgb scene like ITMMainEngine::ProcessFrame does (the scene of mesh_ply_demo), then ITMSceneQueryEngine_HIP samples sdf,
// gradient, normal, colour, weight and flags on a lattice of points across the wall and casts a fan of rays at it.
//   scene_query_demo
// Prints digests of the results as JSON; tests/test_scene_query.py builds the same scene and the same points and rays through the Python
// binding and compares.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s_rgb V;
typedef ITMVoxelBlockHash I;

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

int main() {
  const int W = 160, H = 120, P = W * H;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMScene<V, I> scene(&params);
  ITMDenseMapper_HIP<V, I> mapper;
  ITMVisualisationEngine_HIP<V, I> vis(&scene);
  ITMTrackingController_HIP<V, I> controller(&vis);
  mapper.ResetScene(&scene);
  ITMRenderState* rs = vis.CreateRenderState(Vector2i{W, H});

  std::vector<float> depth(P);
  std::vector<uint8_t> rgb((size_t)P * 4);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      depth[x + y * W] = 1.5f + 0.002f * (float)((x * 7 + y * 13) % 50);
      uint8_t* c = &rgb[(size_t)(x + y * W) * 4];
      c[0] = (uint8_t)((x * 3) & 255); c[1] = (uint8_t)((y * 5) & 255); c[2] = (uint8_t)((x + y) & 255); c[3] = 255;
    }
  void *dDepth, *dRgb, *dPts, *dNrm;
  check(itm_dev_malloc(&dDepth, P * 4), "malloc"); check(itm_dev_malloc(&dRgb, P * 4), "malloc");
  check(itm_dev_malloc(&dPts, P * 16), "malloc"); check(itm_dev_malloc(&dNrm, P * 16), "malloc");
  check(itm_memcpy_h2d(dDepth, depth.data(), P * 4, nullptr), "h2d");
  check(itm_memcpy_h2d(dRgb, rgb.data(), P * 4, nullptr), "h2d");

  ITMView view;
  view.calib.intrinsics_d.SetFrom(145.f, 145.f, 80.f, 60.f);
  view.calib.intrinsics_rgb = view.calib.intrinsics_d;
  view.depth = (const float*)dDepth; view.rgb = (const uint8_t*)dRgb;
  view.depthSize = Vector2i{W, H}; view.rgbSize = Vector2i{W, H};
  ITMTrackingState ts;
  ts.pointCloud_locations = (float*)dPts; ts.pointCloud_colours = (float*)dNrm;
  for (int k = 0; k < 2; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.01f * k, 0, 0, 1};
    ts.pose_d.SetM(M);
    controller.Track(&ts, &view);
    mapper.ProcessFrame(&view, &ts, &scene, rs);
    controller.Prepare(&ts, &view, rs);
  }

  // a lattice of 41 x 31 x 21 points in metres around the wall (z = 1.5 .. 1.6 m), and 41 x 31 rays from the first camera through it
  const int NX = 41, NY = 31, NZ = 21;
  const uint32_t n = NX * NY * NZ, nr = NX * NY;
  std::vector<float> points((size_t)n * 3), rays((size_t)nr * 8);
  for (int k = 0; k < NZ; ++k)
    for (int j = 0; j < NY; ++j)
      for (int i = 0; i < NX; ++i) {
        float* p = &points[(size_t)(i + NX * (j + NY * k)) * 3];
        p[0] = -0.6f + 0.03f * (float)i; p[1] = -0.45f + 0.03f * (float)j; p[2] = 1.45f + 0.01f * (float)k;
      }
  for (int j = 0; j < NY; ++j)
    for (int i = 0; i < NX; ++i) {
      float* r = &rays[(size_t)(i + NX * j) * 8];
      const float dx = -0.4f + 0.02f * (float)i, dy = -0.3f + 0.02f * (float)j;      // direction (dx, dy, 1), not normalised
      r[0] = 0.5f * dx; r[1] = 0.5f * dy; r[2] = 0.5f; r[3] = 0.5f;
      r[4] = 3.0f * dx; r[5] = 3.0f * dy; r[6] = 3.0f; r[7] = 3.0f;
    }
  void *dPoints, *dRays, *dHits, *dSdf, *dGrad, *dNormal, *dColour, *dWeight, *dFlags;
  check(itm_dev_malloc(&dPoints, points.size() * 4), "malloc"); check(itm_dev_malloc(&dRays, rays.size() * 4), "malloc");
  check(itm_dev_malloc(&dHits, (size_t)nr * 16), "malloc"); check(itm_dev_malloc(&dSdf, (size_t)n * 4), "malloc");
  check(itm_dev_malloc(&dGrad, (size_t)n * 12), "malloc"); check(itm_dev_malloc(&dNormal, (size_t)n * 12), "malloc");
  check(itm_dev_malloc(&dColour, (size_t)n * 4), "malloc"); check(itm_dev_malloc(&dWeight, n), "malloc");
  check(itm_dev_malloc(&dFlags, (size_t)n * 4), "malloc");
  check(itm_memcpy_h2d(dPoints, points.data(), points.size() * 4, nullptr), "h2d");
  check(itm_memcpy_h2d(dRays, rays.data(), rays.size() * 4, nullptr), "h2d");
  check(itm_stream_synchronize(nullptr), "sync");

  ITMSceneQueryEngine_HIP<V, I> query;
  itm_query_out out;
  std::memset(&out, 0, sizeof out);
  out.sdf = (float*)dSdf; out.gradient = (float*)dGrad; out.normal = (float*)dNormal; out.colour = (uint8_t*)dColour;
  out.weight = (uint8_t*)dWeight; out.flags = (uint32_t*)dFlags;
  query.QueryPoints(&scene, (const float*)dPoints, n, out);
  query.CastRays(&scene, (const float*)dRays, nr, (float*)dHits);

  const std::vector<float> sdf = fetch<float>(dSdf, n), grad = fetch<float>(dGrad, (size_t)n * 3), normal = fetch<float>(dNormal, (size_t)n * 3);
  const std::vector<uint8_t> colour = fetch<uint8_t>(dColour, (size_t)n * 4), weight = fetch<uint8_t>(dWeight, n);
  const std::vector<uint32_t> flags = fetch<uint32_t>(dFlags, n);
  std::vector<float> hits = fetch<float>(dHits, (size_t)nr * 4);
  uint32_t nHits = 0, allCorners = 0;
  for (uint32_t i = 0; i < nr; ++i) {
    if (hits[4 * i + 3] > 0.0f) ++nHits;
    else hits[4 * i] = hits[4 * i + 1] = hits[4 * i + 2] = 0.0f;      // a miss's xyz is unspecified
  }
  for (uint32_t i = 0; i < n; ++i) allCorners += (flags[i] & 2u) ? 1u : 0u;
  printf("{\"points\": %u, \"rays\": %u, \"hits\": %u, \"all_corners\": %u, \"sdf\": \"%016llx\", \"gradient\": \"%016llx\", \"normal\": \"%016llx\", "
         "\"colour\": \"%016llx\", \"weight\": \"%016llx\", \"flags\": \"%016llx\", \"hit_points\": \"%016llx\"}\n",
         n, nr, nHits, allCorners, (unsigned long long)fnv(sdf.data(), sdf.size() * 4), (unsigned long long)fnv(grad.data(), grad.size() * 4),
         (unsigned long long)fnv(normal.data(), normal.size() * 4), (unsigned long long)fnv(colour.data(), colour.size()),
         (unsigned long long)fnv(weight.data(), weight.size()), (unsigned long long)fnv(flags.data(), flags.size() * 4),
         (unsigned long long)fnv(hits.data(), hits.size() * 4));
  delete rs;
  for (void* p : {dDepth, dRgb, dPts, dNrm, dPoints, dRays, dHits, dSdf, dGrad, dNormal, dColour, dWeight, dFlags}) itm_dev_free(p);
  return 0;
}
