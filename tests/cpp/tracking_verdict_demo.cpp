// The tracking verdict through the C++ adapter: ITMMainEngine_HIP with ITMLibSettings::useTrackingVerdict judges every frame's pose
// against the fused volume, fuses GOOD frames only and -- with useRelocalisation -- recovers a FAILED pose from a keyframe.
//   tracking_verdict_demo <file> [tracker=external|icp] [verdict=0|1] [reloc=0|1] [delay=N] [skip=K] [digests=0|1]
// file: int32 {w, h, n}, float intr[4], int16 raw[n*h*w], float poses[n*16].  tracker=external: poses[k] is written into pose_d before
//       frame k, as a host with its own pose source does; tracker=icp: poses[0] only.  skip=K: frame K is never shown to the engine.
//       digests=1: the scene's digest after every frame too.
// Prints one JSON line: per frame the result, the counts, pose_d, whether the frame was fused, the keyframes and recoveries so far;
// then the keyframe poses and the SHA-256 of the hash table and the voxel blocks.  tests/test_pose_quality.py compares runs with each
// other and with the same frames through the Python binding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s V;
typedef ITMVoxelBlockHash I;

template <class T> static bool rd(FILE* f, T* dst, size_t n) { return fread(dst, sizeof(T), n, f) == n; }

// SHA-256 (FIPS 180-4) of a sequence of buffers
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint8_t block[64];
  size_t fill = 0;
  uint64_t bytes = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void compress(const uint8_t* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void update(const void* data, size_t n) {
    const uint8_t* p = (const uint8_t*)data;
    bytes += n;
    while (n) {
      if (fill == 0 && n >= 64) { compress(p); p += 64; n -= 64; continue; }
      const size_t take = (64 - fill < n) ? 64 - fill : n;
      memcpy(block + fill, p, take);
      fill += take; p += take; n -= take;
      if (fill == 64) { compress(block); fill = 0; }
    }
  }
  std::string hex() {
    const uint64_t bits = bytes * 8;
    const uint8_t one = 0x80, zero = 0;
    update(&one, 1);
    while (fill != 56) update(&zero, 1);
    uint8_t len[8];
    for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
    update(len, 8);
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return std::string(out);
  }
};

// SHA-256 of the hash table and the voxel blocks
static std::string scene_digest(const itm_scene* scene) {
  Sha256 sha;
  const int which[2] = {ITM_BUF_HASH_ENTRIES, ITM_BUF_VOXEL_BLOCKS};
  for (int b : which) {
    const size_t n = itm_buffer_bytes(scene, nullptr, b);
    std::vector<uint8_t> host(n);
    check(itm_download(scene, nullptr, b, host.data(), n, nullptr), "download");
    sha.update(host.data(), n);
  }
  return sha.hex();
}

static void print_pose(const float* M) {
  printf("[");
  for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", M[i]);
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <file> [tracker=external|icp] [verdict=0|1] [reloc=0|1] [delay=N] [skip=K] [digests=0|1]\n", argv[0]); return 2; }
  bool icp = false, verdict = true, reloc = false, digests = false;
  int delay = 10, skip = -1;
  for (int i = 2; i < argc; ++i) {
    const std::string a(argv[i]);
    const size_t eq = a.find('=');
    if (eq == std::string::npos) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    const std::string key = a.substr(0, eq), val = a.substr(eq + 1);
    if (key == "tracker") icp = val == "icp";
    else if (key == "verdict") verdict = atoi(val.c_str()) != 0;
    else if (key == "reloc") reloc = atoi(val.c_str()) != 0;
    else if (key == "delay") delay = atoi(val.c_str());
    else if (key == "skip") skip = atoi(val.c_str());
    else if (key == "digests") digests = atoi(val.c_str()) != 0;
    else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t hd[3]; float intr[4];
  if (!rd(f, hd, 3) || !rd(f, intr, 4)) return 2;
  const int W = hd[0], H = hd[1], N = hd[2];
  const size_t P = (size_t)W * H;
  std::vector<int16_t> raw((size_t)N * P);
  std::vector<float> poses((size_t)N * 16);
  if (!rd(f, raw.data(), raw.size()) || !rd(f, poses.data(), poses.size())) return 2;
  fclose(f);

  ITMLibSettings st;
  st.trackerType = icp ? ITMLibSettings::TRACKER_ICP : ITMLibSettings::TRACKER_EXTERNAL;
  st.noHierarchyLevels = 3;      // five levels leave too few points on the coarsest at 160 x 120
  st.trackingRegime[0] = ITM_TRACKER_ITERATION_BOTH; st.trackingRegime[1] = ITM_TRACKER_ITERATION_BOTH; st.trackingRegime[2] = ITM_TRACKER_ITERATION_ROTATION;
  st.useTrackingVerdict = verdict;
  st.relocFusionDelay = delay;
  st.useRelocalisation = reloc;
  st.relocHarvestingThreshold = 0.05f;
  st.relocCapacity = 256;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(intr[0], intr[1], intr[2], intr[3]);
  calib.intrinsics_rgb = calib.intrinsics_d;
  ITMMainEngine_HIP<V, I> engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x2000);
  ITMTrackingState* ts = engine.GetTrackingState();

  void* dRaw;
  check(itm_dev_malloc(&dRaw, P * 2), "malloc");
  printf("{\"frames\": [");
  bool first = true;
  for (int k = 0; k < N; ++k) {
    if (k == skip) continue;
    check(itm_memcpy_h2d(dRaw, raw.data() + (size_t)k * P, P * 2, nullptr), "h2d");
    if (!icp || k == 0) ts->pose_d.SetM(poses.data() + (size_t)k * 16);
    engine.ProcessFrame(nullptr, (const int16_t*)dRaw);
    const itm_pose_quality& q = engine.GetPoseQuality();
    printf("%s{\"k\": %d, \"result\": %d, \"stats\": [%d, %d, %d, %d, %.17g, %.17g], \"fused\": %d, \"keyframes\": %d, \"recoveries\": %d, \"pose\": ", first ? "" : ", ", k,
           (int)engine.GetTrackingResult(), q.noPixels, q.noValid, q.noKnown, q.noInliers, q.sumSqKnown, q.sumSqInliers, engine.LastFrameFused() ? 1 : 0,
           engine.GetRelocaliser() ? engine.GetRelocaliser()->NumKeyframes() : 0, engine.GetRelocalisationCount());
    print_pose(ts->pose_d.GetM());
    if (digests) printf(", \"digest\": \"%s\"", scene_digest(engine.GetScene()->handle).c_str());
    printf("}");
    first = false;
  }
  printf("], \"keyframe_poses\": [");
  if (engine.GetRelocaliser())
    for (int i = 0; i < engine.GetRelocaliser()->NumKeyframes(); ++i) {
      if (i) printf(", ");
      print_pose(engine.GetRelocaliser()->RetrievePose(i).GetM());
    }
  printf("], \"digest\": \"");
  printf("%s\"}\n", scene_digest(engine.GetScene()->handle).c_str());
  itm_dev_free(dRaw);
  return 0;
}
