// Loses the pose and finds it again through the C++ adapter: ITMMainEngine_HIP with ITMLibSettings::useRelocalisation tracks (ICP, three
// levels) and fuses a sequence of raw depth frames, harvesting keyframes as it goes; then pose_d is overwritten with a pose 30 cm off
// and Relocalise() is called on a frame of the sequence.
//   relocaliser_demo <file>
// file: int32 {w, h, n, query}, float intr[4], int16 raw[n*h*w], float poses[n*16] (poses[0] is the first frame's pose; the others are
//       the truth, for the caller).  Prints one JSON line: the id harvested per frame, the keyframe Relocalise chose, its pose, the
//       refined pose and a digest of the ICP points left for the next frame; tests/test_relocaliser.py makes the same calls through the
//       Python binding and compares.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s V;
typedef ITMVoxelBlockHash I;

template <class T> static bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[4]; float intr[4];
  if (!rd(f, hd, 4) || !rd(f, intr, 4)) return 2;
  const int W = hd[0], H = hd[1], N = hd[2], query = hd[3];
  const size_t P = (size_t)W * H;
  std::vector<int16_t> raw((size_t)N * P);
  std::vector<float> poses((size_t)N * 16);
  if (!rd(f, raw.data(), raw.size()) || !rd(f, poses.data(), poses.size())) return 2;
  fclose(f);

  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_ICP;
  st.noHierarchyLevels = 3;      // five levels leave too few points on the coarsest at 160 x 120
  st.trackingRegime[0] = ITM_TRACKER_ITERATION_BOTH; st.trackingRegime[1] = ITM_TRACKER_ITERATION_BOTH; st.trackingRegime[2] = ITM_TRACKER_ITERATION_ROTATION;
  st.useRelocalisation = true;
  st.relocHarvestingThreshold = 0.05f;
  st.relocCapacity = 256;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  calib.intrinsics_rgb = calib.intrinsics_d;
  ITMMainEngine_HIP<V, I> engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H});
  ITMRelocaliser_HIP* reloc = engine.GetRelocaliser();
  ITMTrackingState* ts = engine.GetTrackingState();

  void* dRaw;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc");
  // nothing to relocalise against yet: -1, and the pose stays
  check(itm_memcpy_h2d(dRaw, raw.data(), P * 2, nullptr), "h2d");
  ts->pose_d.SetM(poses.data());
  const int none = engine.Relocalise(nullptr, (const int16_t*)dRaw);
  const bool kept = memcmp(ts->pose_d.GetM(), poses.data(), 64) == 0;

  std::vector<int> added;
  for (int k = 0; k < N; ++k) {
    check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    const int before = reloc->NumKeyframes();
    engine.ProcessFrame(nullptr, (const int16_t*)dRaw);
    added.push_back(reloc->NumKeyframes() > before ? before : -1);
  }

  // lost: 30 cm off
  float lost[16];
  memcpy(lost, ts->pose_d.GetM(), 64);
  lost[12] += 0.3f;
  ts->pose_d.SetM(lost);
  check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)query * P, P * 2, nullptr), "h2d");
  const int keyframe = engine.Relocalise(nullptr, (const int16_t*)dRaw);
  if (keyframe < 0) { fprintf(stderr, "no keyframe\n"); return 1; }
  const ITMPose kfPose = reloc->RetrievePose(keyframe);
  int nearest; float distance;
  reloc->ProcessFrame(engine.GetView()->depth, nullptr, 1, &nearest, &distance, false);      // the distance Relocalise saw

  std::vector<float> pts(P * 4);
  check(itm_memcpy_d2h(pts.data(), ts->pointCloud_locations, P * 16, nullptr), "d2h");
  check(itm_stream_synchronize(nullptr), "sync");
  printf("{\"none\": %d, \"kept\": %d, \"count\": %d, \"keyframe\": %d, \"nearest\": %d, \"dist\": %.9g, \"added\": [", none, kept ? 1 : 0, reloc->NumKeyframes(), keyframe,
         nearest, (double)distance);
  for (size_t i = 0; i < added.size(); ++i) printf("%s%d", i ? ", " : "", added[i]);
  printf("], \"keyframe_pose\": [");
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", kfPose.GetM()[i]);
  printf("], \"pose\": [");
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", ts->pose_d.GetM()[i]);
  printf("], \"age\": %d, \"points\": [", ts->age_pointCloud);
  // the ICP points as their bit patterns' sum and xor: a digest the caller can form with numpy
  uint64_t sum = 0; uint32_t x = 0;
  for (size_t i = 0; i < pts.size(); ++i) { uint32_t b; memcpy(&b, &pts[i], 4); sum += b; x ^= b; }
  printf("%llu, %u]}\n", (unsigned long long)sum, x);
  itm_dev_free(dRaw);
  return 0;
}
