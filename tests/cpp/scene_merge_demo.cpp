// Drives ITMSceneMergeEngine_HIP::MergeScene and ITMMainEngine_HIP::MergeSceneFrom (include/itm_hip_engines.hpp; itm_scene_merge).
//   scene_merge_demo             two small hash scenes (160x120, 1 cm voxels, flat walls at 1.5 m and 1.52 m seen from shifted cameras);
//                                the blocks of B's visible list are merged into A.  Prints one JSON line: the statistics and a digest
//                                of the merged table and voxels -- sum of word[i] * (2 i + 1) modulo 2^64 over the 32-bit words --
//                                which tests/test_scene_merge.py computes for the same merge through the Python binding.
//   scene_merge_demo --engines   two main engines (poses from outside), two frames each, then A.MergeSceneFrom(B): the statistics.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

static const int W = 160, H = 120, P = W * H;

static unsigned long long digest(itm_scene* s, int which) {
  const size_t n = itm_buffer_bytes(s, nullptr, which);
  std::vector<uint32_t> buf(n / 4);
  check(itm_download(s, nullptr, which, buf.data(), n, nullptr), "download");
  unsigned long long d = 0;
  for (size_t i = 0; i < buf.size(); ++i) d += (unsigned long long)buf[i] * (2ull * i + 1ull);
  return d;
}

static void print_stats(const itm_merge_stats& m) {
  printf("\"rounds\": %d, \"considered\": %d, \"alreadyPresent\": %d, \"allocated\": %d, \"combined\": %d, \"unserved\": %d, \"srcWithoutBlock\": %d, \"dstSwappedOut\": %d",
         m.rounds, m.considered, m.alreadyPresent, m.allocated, m.combined, m.unserved, m.srcWithoutBlock, m.dstSwappedOut);
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
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  Scene a(&params, 0x2000, 0x1000, 0x400), b(&params, 0x2000, 0x1000, 0x400);
  ITMSceneReconstructionEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> reco;
  reco.ResetScene(&a); reco.ResetScene(&b);
  ITMVisualisationEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> visA(&a), visB(&b);
  ITMRenderState* rsA = visA.CreateRenderState(Vector2i{W, H});
  ITMRenderState* rsB = visB.CreateRenderState(Vector2i{W, H});
  void *depthBuf, *pts, *col;
  check(itm_dev_malloc(&depthBuf, (size_t)P * 4), "malloc"); check(itm_dev_malloc(&pts, (size_t)P * 16), "malloc"); check(itm_dev_malloc(&col, (size_t)P * 16), "malloc");
  ITMTrackingState ts;
  ts.pointCloud_locations = (float*)pts; ts.pointCloud_colours = (float*)col;
  fill(&a, &visA, rsA, 1.5f, 0.0f, depthBuf, &ts);
  fill(&b, &visB, rsB, 1.52f, -0.4f, depthBuf, &ts);
  itm_merge_stats m;
  ITMSceneMergeEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> merger;
  merger.MergeScene(&a, &b, rsB, &m);
  check(itm_stream_synchronize(nullptr), "sync");
  itm_counters c;
  check(itm_get_counters(a.handle, nullptr, &c, nullptr), "counters");
  printf("{");
  print_stats(m);
  printf(", \"lastFreeBlockId\": %d, \"lastFreeExcessListId\": %d, \"table\": \"%016llx\", \"voxels\": \"%016llx\"}\n", c.lastFreeBlockId, c.lastFreeExcessListId,
         digest(a.handle, ITM_BUF_HASH_ENTRIES), digest(a.handle, ITM_BUF_VOXEL_BLOCKS));
  delete rsA; delete rsB;
  itm_dev_free(depthBuf); itm_dev_free(pts); itm_dev_free(col);
  return 0;
}

static int engines() {
  typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine a(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000), b(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000);
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  Engine* both[2] = {&a, &b};
  for (int e = 0; e < 2; ++e) {
    std::vector<int16_t> raw((size_t)P, (int16_t)(e ? 1520 : 1500));
    check(itm_memcpy_h2d(dRaw, raw.data(), (size_t)P * 2, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    for (int k = 0; k < 2; ++k) {
      float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      M[12] = (e ? -0.4f : 0.0f) - 0.01f * (float)k;
      both[e]->GetTrackingState()->pose_d.SetM(M);
      both[e]->ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    }
  }
  itm_counters before, after, src;
  check(itm_get_counters(a.GetScene()->handle, nullptr, &before, nullptr), "counters");
  check(itm_get_counters(b.GetScene()->handle, nullptr, &src, nullptr), "counters");
  itm_merge_stats m;
  a.MergeSceneFrom(b, &m);
  check(itm_stream_synchronize(nullptr), "sync");
  check(itm_get_counters(a.GetScene()->handle, nullptr, &after, nullptr), "counters");
  a.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);      // the merged scene goes on living
  printf("{");
  print_stats(m);
  printf(", \"blocks_before\": %d, \"blocks_after\": %d, \"src_blocks\": %d}\n", 0x4000 - 1 - before.lastFreeBlockId, 0x4000 - 1 - after.lastFreeBlockId, 0x4000 - 1 - src.lastFreeBlockId);
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  try {
    return (argc > 1 && !strcmp(argv[1], "--engines")) ? engines() : scenes();
  } catch (const std::exception& e) {
    fprintf(stderr, "scene_merge_demo: %s\n", e.what());
    return 1;
  }
}
