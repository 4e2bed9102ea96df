// Drives ITMSceneResampleEngine_HIP::ResampleScene and ITMMainEngine_HIP::MergeSceneFrom(other, thisFromOther)
// (include/itm_hip_engines.hpp; itm_rigid_quantise + itm_scene_resample).
//   scene_resample_demo                    two small hash scenes of 1 cm voxels (160x120, mu 4 cm): A holds a flat wall at 1.5 m seen by two
//                                          frames, C a wall at 1.52 m seen from 0.4 m aside.  The blocks of A's visible list are resampled
//                                          into C under a rotation of 0.3 rad about (1, 2, 3) with a fractional translation.  Prints one
//                                          JSON line: the statistics, the counters and a digest of C's table and voxels -- sum of
//                                          word[i] * (2 i + 1) modulo 2^64 over the 32-bit words -- which tests/test_scene_resample.py
//                                          computes for the same call through the Python binding.
//   scene_resample_demo --engines DA DB    two main engines (poses from outside), two frames each; their scenes are saved to DA and DB
//                                          (itm_scene_save), then the second is merged into the first under the same transform
//                                          (MergeSceneFrom): statistics and digests, and the first engine goes on taking frames.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

static const int W = 160, H = 120, P = W * H;
// dstFromSrc, column-major: rotation by 0.3 rad about (1, 2, 3) / sqrt(14), translation (0.1234, -0.0567, 0.0891) m
static const float kTransform[16] = {0.958526731f, 0.243323788f, -0.148391441f, 0.0f, -0.230562791f, 0.968097508f, 0.0981226042f, 0.0f,
                                     0.167532951f, -0.0598395914f, 0.984048724f, 0.0f, 0.123400003f, -0.0566999987f, 0.0891000032f, 1.0f};

static unsigned long long digest(itm_scene* s, int which) {
  const size_t n = itm_buffer_bytes(s, nullptr, which);
  std::vector<uint32_t> buf(n / 4);
  check(itm_download(s, nullptr, which, buf.data(), n, nullptr), "download");
  unsigned long long d = 0;
  for (size_t i = 0; i < buf.size(); ++i) d += (unsigned long long)buf[i] * (2ull * i + 1ull);
  return d;
}

static void print_result(const itm_resample_stats& m, itm_scene* dst) {
  check(itm_stream_synchronize(nullptr), "sync");
  itm_counters c;
  check(itm_get_counters(dst, nullptr, &c, nullptr), "counters");
  printf("{\"rounds\": %d, \"considered\": %d, \"candidates\": %d, \"alreadyPresent\": %d, \"allocated\": %d, \"resampled\": %d, \"unserved\": %d, \"srcWithoutBlock\": %d, "
         "\"dstSwappedOut\": %d, \"outOfRange\": %d",
         m.rounds, m.considered, m.candidates, m.alreadyPresent, m.allocated, m.resampled, m.unserved, m.srcWithoutBlock, m.dstSwappedOut, m.outOfRange);
  printf(", \"lastFreeBlockId\": %d, \"lastFreeExcessListId\": %d, \"table\": \"%016llx\", \"voxels\": \"%016llx\"}\n", c.lastFreeBlockId, c.lastFreeExcessListId,
         digest(dst, ITM_BUF_HASH_ENTRIES), digest(dst, ITM_BUF_VOXEL_BLOCKS));
}

typedef ITMScene<ITMVoxel_s, ITMVoxelBlockHash> Scene;

// two frames of a flat wall at `z` metres, the camera shifted by tx0 (+ 1 cm per frame) along x
static void fill(Scene* scene, ITMVisualisationEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>* vis, ITMRenderState* rs, float z, float tx0, void* depthBuf, ITMTrackingState* ts) {
  ITMSceneReconstructionEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> reco;
  std::vector<float> depth((size_t)P, z);
  check(itm_memcpy_h2d(depthBuf, depth.data(), (size_t)P * 4, nullptr), "h2d");
  check(itm_stream_synchronize(nullptr), "sync");
  ITMView view;
  view.depth = (const float*)depthBuf; view.depthSize = Vector2i{W, H}; view.rgbSize = Vector2i{W, H};
  view.calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  view.calib.intrinsics_rgb = view.calib.intrinsics_d;
  for (int k = 0; k < 2; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    M[12] = tx0 - 0.01f * (float)k;
    ts->pose_d.SetM(M);
    reco.AllocateSceneFromDepth(scene, &view, ts, rs);
    reco.IntegrateIntoScene(scene, &view, ts, rs);
    vis->CreateExpectedDepths(&ts->pose_d, &view.calib.intrinsics_d, rs);
    vis->CreateICPMaps(&view, ts, rs);
  }
}

static int scenes() {
  ITMSceneParams params(0.04f, 100, 0.01f, 0.35f, 3.0f, false);
  Scene a(&params, 0x2000, 0x1000, 0x400), c(&params, 0x2000, 0x1000, 0x400);
  ITMSceneReconstructionEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> reco;
  reco.ResetScene(&a); reco.ResetScene(&c);
  ITMVisualisationEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> visA(&a), visC(&c);
  ITMRenderState* rsA = visA.CreateRenderState(Vector2i{W, H});
  ITMRenderState* rsC = visC.CreateRenderState(Vector2i{W, H});
  void *depthBuf, *pts, *col;
  check(itm_dev_malloc(&depthBuf, (size_t)P * 4), "malloc"); check(itm_dev_malloc(&pts, (size_t)P * 16), "malloc"); check(itm_dev_malloc(&col, (size_t)P * 16), "malloc");
  ITMTrackingState ts;
  ts.pointCloud_locations = (float*)pts; ts.pointCloud_colours = (float*)col;
  fill(&a, &visA, rsA, 1.5f, 0.0f, depthBuf, &ts);
  fill(&c, &visC, rsC, 1.52f, -0.4f, depthBuf, &ts);
  itm_resample_stats m;
  ITMSceneResampleEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> resampler;
  resampler.ResampleScene(&c, &a, Matrix4f(kTransform), rsA, &m);
  print_result(m, c.handle);
  delete rsA; delete rsC;
  itm_dev_free(depthBuf); itm_dev_free(pts); itm_dev_free(col);
  return 0;
}

static int engines(const char* dirA, const char* dirB) {
  typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  ITMSceneParams params(0.04f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine a(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000), b(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000);
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  Engine* both[2] = {&a, &b};
  for (int e = 0; e < 2; ++e) {
    std::vector<int16_t> raw((size_t)P);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) raw[(size_t)y * W + x] = (int16_t)((e ? 1520 : 1500) + ((x / 40 + y / 40) % 2) * 60);      // a wall with 6 cm tiles
    check(itm_memcpy_h2d(dRaw, raw.data(), (size_t)P * 2, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    for (int k = 0; k < 2; ++k) {
      float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      M[12] = (e ? -0.4f : 0.0f) - 0.01f * (float)k;
      both[e]->GetTrackingState()->pose_d.SetM(M);
      both[e]->ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    }
  }
  check(itm_scene_save(a.GetScene()->handle, nullptr, dirA, nullptr), "itm_scene_save");
  check(itm_scene_save(b.GetScene()->handle, nullptr, dirB, nullptr), "itm_scene_save");
  itm_resample_stats m;
  a.MergeSceneFrom(b, Matrix4f(kTransform), &m);
  print_result(m, a.GetScene()->handle);
  a.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);      // the merged scene goes on living
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc > 3 && !strcmp(argv[1], "--engines")) return engines(argv[2], argv[3]);
    return scenes();
  } catch (const std::exception& e) {
    fprintf(stderr, "scene_resample_demo: %s\n", e.what());
    return 1;
  }
}
