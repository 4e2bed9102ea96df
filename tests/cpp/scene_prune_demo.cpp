// Drives ITMMainEngine_HIP with ITMLibSettings::pruneEveryNFrames and ITMScenePruneEngine_HIP::PruneScene (include/itm_hip_engines.hpp;
// itm_scene_prune).
//   scene_prune_demo N    one main engine (poses from outside; 160x120, 1 cm voxels, a flat wall at 1.5 m seen from a camera that moves
//                         5 cm per frame), six frames, the scene pruned after every N-th (0: never) with empty, free and once-seen
//                         blocks as candidates and no protection: the columns of blocks a frame has just uncovered go again.
//                         Prints one JSON line: the blocks the engine's prunes dropped, the counters, a digest of the table and of
//                         the voxels -- sum of word[i] * (2 i + 1) modulo 2^64 over the 32-bit words --
//                         and the statistics of a dry run through the prune engine at the end; tests/test_scene_prune.py reaches the
//                         same state with the same calls through the Python binding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

static const int W = 160, H = 120, P = W * H, FRAMES = 6;

static unsigned long long digest(itm_scene* s, int which) {
  const size_t n = itm_buffer_bytes(s, nullptr, which);
  std::vector<uint32_t> buf(n / 4);
  check(itm_download(s, nullptr, which, buf.data(), n, nullptr), "download");
  unsigned long long d = 0;
  for (size_t i = 0; i < buf.size(); ++i) d += (unsigned long long)buf[i] * (2ull * i + 1ull);
  return d;
}

static int run(int every) {
  typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  st.pruneEveryNFrames = every;
  st.pruneConfig.classes = ITM_PRUNE_EMPTY | ITM_PRUNE_FREE | ITM_PRUNE_WEAK;
  st.pruneConfig.weakMaxW = 1;
  st.pruneConfig.protect = 0;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine e(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000);
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  std::vector<int16_t> raw((size_t)P, (int16_t)1500);
  check(itm_memcpy_h2d(dRaw, raw.data(), (size_t)P * 2, nullptr), "h2d");
  check(itm_stream_synchronize(nullptr), "sync");
  int prunes = 0, dropped = 0, removed = 0;
  for (int k = 0; k < FRAMES; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    M[12] = -0.05f * (float)k;
    e.GetTrackingState()->pose_d.SetM(M);
    e.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    if (every > 0 && (k + 1) % every == 0) { ++prunes; dropped += e.GetLastPruneStats().dropped; removed += e.GetLastPruneStats().visibleRemoved; }
  }
  itm_prune_config dry = st.pruneConfig;
  dry.dryRun = 1;
  itm_prune_stats d;
  ITMScenePruneEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>().PruneScene(e.GetScene(), &dry, &d);
  itm_counters c;
  check(itm_get_counters(e.GetScene()->handle, e.GetRenderState()->handle, &c, nullptr), "counters");
  printf("{\"prunes\": %d, \"dropped\": %d, \"visibleRemoved\": %d, \"lastFreeBlockId\": %d, \"lastFreeExcessListId\": %d, \"noVisibleEntries\": %d, "
         "\"table\": \"%016llx\", \"voxels\": \"%016llx\", \"dry_considered\": %d, \"dry_candidates\": %d, \"dry_dropped\": %d}\n",
         prunes, dropped, removed, c.lastFreeBlockId, c.lastFreeExcessListId, c.noVisibleEntries, digest(e.GetScene()->handle, ITM_BUF_HASH_ENTRIES),
         digest(e.GetScene()->handle, ITM_BUF_VOXEL_BLOCKS), d.considered, d.candidates, d.dropped);
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  try {
    return run(argc > 1 ? atoi(argv[1]) : 2);
  } catch (const std::exception& e) {
    fprintf(stderr, "scene_prune_demo: %s\n", e.what());
    return 1;
  }
}
