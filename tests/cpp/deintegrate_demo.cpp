// Drives ITMMainEngine_HIP::ReintegrateFrame / RemoveFrame (include/itm_hip_engines.hpp; itm_deintegrate_from_scene).
//   deintegrate_demo DIR MODE J   DIR holds frames.bin (int16 [N][120][160], raw depth in mm) and poses.bin (float [N + 1][16]: the pose
//                                 of every frame, then the corrected pose of frame J).  One main engine (poses from outside, 5 mm voxels)
//                                 fuses the N frames; then frame J is
//                                   MODE reintegrate   taken out under its pose and fused again under the corrected one,
//                                   MODE same          taken out and fused again under the pose it had,
//                                   MODE remove        taken out.
//                                 Prints one JSON line: the de-integration's statistics, the counters, and a digest of every scene buffer
//                                 and of the live render state's visible list -- sum of word[i] * (2 i + 1) modulo 2^64 over the 32-bit
//                                 words; tests/test_deintegrate.py reaches the same state with the calls made by hand through the Python
//                                 binding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

static const int W = 160, H = 120, P = W * H;

template <class T>
static std::vector<T> read_all(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)n / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fclose(f); throw std::runtime_error("short read of " + path); }
  fclose(f);
  return v;
}

static unsigned long long digest(itm_scene* s, itm_render_state* rs, int which) {
  const size_t n = itm_buffer_bytes(s, rs, which);
  std::vector<uint32_t> buf((n + 3) / 4, 0u);
  check(itm_download(s, rs, which, buf.data(), n, nullptr), "download");
  unsigned long long d = 0;
  for (size_t i = 0; i < buf.size(); ++i) d += (unsigned long long)buf[i] * (2ull * i + 1ull);
  return d;
}

static int run(const std::string& dir, const std::string& mode, int j) {
  typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;
  const std::vector<int16_t> frames = read_all<int16_t>(dir + "/frames.bin");
  const std::vector<float> poses = read_all<float>(dir + "/poses.bin");
  const int n = (int)(frames.size() / (size_t)P);
  if (n < 1 || (int)poses.size() != (n + 1) * 16 || j < 0 || j >= n) throw std::runtime_error("frames.bin / poses.bin do not fit");
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  ITMSceneParams params(0.02f, 100, 0.005f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine e(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x4000);
  void *dRaw, *dRgb, *dDepth;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc"); check(itm_dev_malloc(&dDepth, (size_t)P * 4), "malloc");
  for (int k = 0; k < n; ++k) {
    check(itm_memcpy_h2d(dRaw, frames.data() + (size_t)k * P, (size_t)P * 2, nullptr), "h2d");
    check(itm_stream_synchronize(nullptr), "sync");
    e.GetTrackingState()->pose_d.SetM(poses.data() + 16 * k);
    e.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
  }
  // frame J again, in a depth image of the host's own
  check(itm_memcpy_h2d(dRaw, frames.data() + (size_t)j * P, (size_t)P * 2, nullptr), "h2d");
  check(itm_convert_depth_affine((const int16_t*)dRaw, (float*)dDepth, W, H, 0.001f, 0.0f, nullptr), "convert");
  ITMView frame = *e.GetView();
  frame.depth = (const float*)dDepth;
  ITMPose oldPose, newPose;
  oldPose.SetM(poses.data() + 16 * j);
  newPose.SetM(poses.data() + 16 * n);
  const ITMPose live = e.GetTrackingState()->pose_d;
  itm_deintegrate_stats ds;
  if (mode == "reintegrate") e.ReintegrateFrame(&frame, oldPose, newPose, &ds);
  else if (mode == "same") e.ReintegrateFrame(&frame, oldPose, oldPose, &ds);
  else if (mode == "remove") e.RemoveFrame(&frame, oldPose, &ds);
  else throw std::runtime_error("unknown mode " + mode);
  if (memcmp(live.GetM(), e.GetTrackingState()->pose_d.GetM(), 64) != 0) throw std::runtime_error("the tracking pose changed");
  itm_scene* s = e.GetScene()->handle;
  itm_render_state* rs = e.GetRenderState()->handle;
  itm_counters c;
  check(itm_get_counters(s, rs, &c, nullptr), "counters");
  printf("{\"blocks\": %d, \"visited\": %d, \"touched\": %d, \"reset\": %d, \"unobserved\": %d, \"saturated\": %d, \"clamped\": %d, \"coloured\": %d, "
         "\"colourReset\": %d, \"lastFreeBlockId\": %d, \"lastFreeExcessListId\": %d, \"noVisibleEntries\": %d, \"table\": \"%016llx\", \"voxels\": \"%016llx\", "
         "\"excess\": \"%016llx\", \"allocList\": \"%016llx\", \"visibleIds\": \"%016llx\", \"visibleType\": \"%016llx\"}\n",
         ds.blocks, ds.visited, ds.touched, ds.reset, ds.unobserved, ds.saturated, ds.clamped, ds.coloured, ds.colourReset, c.lastFreeBlockId, c.lastFreeExcessListId,
         c.noVisibleEntries, digest(s, nullptr, ITM_BUF_HASH_ENTRIES), digest(s, nullptr, ITM_BUF_VOXEL_BLOCKS), digest(s, nullptr, ITM_BUF_EXCESS_LIST),
         digest(s, nullptr, ITM_BUF_ALLOCATION_LIST), digest(s, rs, ITM_BUF_VISIBLE_IDS), digest(s, rs, ITM_BUF_VISIBLE_TYPE));
  itm_dev_free(dRaw); itm_dev_free(dRgb); itm_dev_free(dDepth);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc < 4) throw std::runtime_error("usage: deintegrate_demo DIR reintegrate|same|remove J");
    return run(argv[1], argv[2], atoi(argv[3]));
  } catch (const std::exception& e) {
    fprintf(stderr, "deintegrate_demo: %s\n", e.what());
    return 1;
  }
}
