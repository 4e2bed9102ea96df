// Drives ITMMainEngine_HIP::GetImage / GetImageDevice / GetImageSize (include/itm_hip_engines.hpp; reference
// Engine/ITMMainEngine.cpp:129-192) over a sequence of raw depth frames read from a file.  Prints one JSON line per frame (pose,
// digests of the tracking maps, as main_engine_demo does) and, after the last frame, one line per GetImage type with the SHA-256
// of the image; the images and the downloads they are compared with are also written to <out dir>.  tests/test_get_image.py
// compares them with the restatement of the colour maps and with the CPU oracle's renders.
//   get_image_demo <sequence file> <out dir>
//   get_image_demo --bench <calls>            GetImageDevice per type after 20 frames of the 640x480 bench scene (4 mm voxels, hash):
//                                             microseconds per call, median of 9 windows of <calls> calls, each ending in a synchronise
// sequence file: int32 hd[16] = {w, h, n, trackerType (0 colour with outside poses, 1 icp, 2 external, 4 weighted icp),
//                useApproximateRaycast, skipPoints, hasPoses, voxelType (0 s, 3 f_rgb), indexType (0 hash, 1 dense), framesFromHost,
//                getImageAfterEveryFrame, freeW, freeH, freeW2, freeH2, sceneDigest},
//                float intr[4], float freePose[16], float freeIntr[4], float freeIntr2[4], int16 raw[n*h*w], float poses[n*16] (if hasPoses),
//                uint8 fusion[n], uint8 mainProcessing[n]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
template <class T> static bool rd(FILE* f, T* dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

// SHA-256 (FIPS 180-4) of a buffer, as lower-case hex
static std::string sha256(const void* data, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
      0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
      0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
      0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
      0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t H[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  std::vector<unsigned char> msg((const unsigned char*)data, (const unsigned char*)data + len);
  msg.push_back(0x80);
  while (msg.size() % 64 != 56) msg.push_back(0);
  for (int i = 7; i >= 0; --i) msg.push_back((unsigned char)(((uint64_t)len * 8) >> (8 * i)));
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  for (size_t off = 0; off < msg.size(); off += 64) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)msg[off + 4 * i] << 24 | (uint32_t)msg[off + 4 * i + 1] << 16 | (uint32_t)msg[off + 4 * i + 2] << 8 | msg[off + 4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
  }
  char hex[65];
  for (int i = 0; i < 8; ++i) snprintf(hex + 8 * i, 9, "%08x", H[i]);
  return std::string(hex);
}

static void dump(const std::string& dir, const char* name, const void* p, size_t n) {
  FILE* f = fopen((dir + "/" + name).c_str(), "wb");
  if (!f || fwrite(p, 1, n, f) != n) { perror(name); exit(2); }
  fclose(f);
}

struct Sequence {
  int32_t hd[16]; float intr[4], freePose[16], freeIntr[4], freeIntr2[4];
  std::vector<int16_t> raw; std::vector<float> poses; std::vector<uint8_t> fusion, mainOn;
};

static const char* kTypeNames[7] = {"original_rgb", "original_depth", "sceneraycast", "freecamera_shaded", "freecamera_colour_from_volume",
                                    "freecamera_colour_from_normal", "unknown"};

template <class V, class I>
static int run(const Sequence& q, const std::string& out) {
  typedef ITMMainEngine_HIP<V, I> Engine;
  const int W = q.hd[0], H = q.hd[1], N = q.hd[2], P = W * H;
  ITMLibSettings st;
  st.trackerType = q.hd[3] == 0 ? ITMLibSettings::TRACKER_COLOR : q.hd[3] == 1 ? ITMLibSettings::TRACKER_ICP : q.hd[3] == 4 ? ITMLibSettings::TRACKER_WICP
                                                                                                                           : ITMLibSettings::TRACKER_EXTERNAL;
  st.useApproximateRaycast = q.hd[4] != 0; st.skipPoints = q.hd[5] != 0;
  const bool fromHost = q.hd[9] != 0, everyFrame = q.hd[10] != 0, colourVoxels = V::kType == ITM_VOXEL_S_RGB || V::kType == ITM_VOXEL_F_RGB;
  ITMSceneParams params(0.02f, 100, 0.005f, 0.35f, 3.0f, false);      // ITMLibSettings.cpp:10
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(q.intr[0], q.intr[1], q.intr[2], q.intr[3]);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H});
  ITMPose freePose; freePose.SetM(q.freePose);
  ITMIntrinsics freeIntr, freeIntr2;
  freeIntr.SetFrom(q.freeIntr[0], q.freeIntr[1], q.freeIntr[2], q.freeIntr[3]);
  freeIntr2.SetFrom(q.freeIntr2[0], q.freeIntr2[1], q.freeIntr2[2], q.freeIntr2[3]);
  const Vector2i freeSize{q.hd[11], q.hd[12]}, freeSize2{q.hd[13], q.hd[14]};

  void *dRaw, *dRgb, *hRaw = nullptr;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  if (fromHost) { check(itm_host_malloc(&hRaw, q.raw.size() * 2), "host malloc"); memcpy(hRaw, q.raw.data(), q.raw.size() * 2); }
  std::vector<uint8_t> rgb((size_t)P * 4);
  for (int i = 0; i < P; ++i) { rgb[4 * i] = (uint8_t)(i % W); rgb[4 * i + 1] = (uint8_t)(i / W); rgb[4 * i + 2] = (uint8_t)((i % W) ^ (i / W)); rgb[4 * i + 3] = 255; }
  check(itm_memcpy_h2d(dRgb, rgb.data(), rgb.size(), nullptr), "h2d");
  check(itm_stream_synchronize(nullptr), "sync");

  // before the first frame: `if (view == NULL) return;` -- the image is not touched
  {
    ITMUChar4Image img(Vector2i{8, 4});
    img.Clear(0x5a);
    engine.GetImage(&img, Engine::InfiniTAM_IMAGE_ORIGINAL_DEPTH);
    bool untouched = img.noDims.x == 8 && img.noDims.y == 4;
    for (size_t i = 0; i < img.dataSize; ++i) untouched = untouched && img.GetData()[i].x == 0x5a && img.GetData()[i].w == 0x5a;
    Vector2i s;
    const bool noDevice = engine.GetImageDevice(&s, Engine::InfiniTAM_IMAGE_SCENERAYCAST) == nullptr && s.x == 0 && s.y == 0;
    printf("{\"before_first_frame_untouched\": %d, \"before_first_frame_no_device_image\": %d}\n", untouched ? 1 : 0, noDevice ? 1 : 0);
  }

  auto every_type = [&](ITMUChar4Image* img, Vector2i size) {
    for (int t = 0; t < 7; ++t) {
      if (t == Engine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME && !colourVoxels) continue;
      img->ChangeDims(size);
      engine.GetImage(img, (typename Engine::GetImageType)t, &freePose, &freeIntr);
    }
  };

  std::vector<float> pts((size_t)P * 4), col((size_t)P * 4); std::vector<uint8_t> live((size_t)P * 4); std::vector<int32_t> ids;
  ITMUChar4Image scratch;
  for (int k = 0; k < N; ++k) {
    ITMTrackingState* ts = engine.GetTrackingState();
    if (q.hd[6]) ts->pose_d.SetM(q.poses.data() + 16 * k);            // the pose source of this fork writes it before the frame
    if (q.fusion[k]) engine.turnOnIntegration(); else engine.turnOffIntegration();
    if (q.mainOn[k]) engine.turnOnMainProcessing(); else engine.turnOffMainProcessing();
    if (fromHost) {
      engine.ProcessFrameFromHost((const uint8_t*)dRgb, (const int16_t*)hRaw + (size_t)k * P, k + 1 < N ? (const int16_t*)hRaw + (size_t)(k + 1) * P : nullptr);
    } else {
      check(itm_memcpy_h2d(dRaw, q.raw.data() + (size_t)k * P, (size_t)P * 2, nullptr), "h2d");
      engine.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    }
    if (everyFrame) every_type(&scratch, freeSize);
    itm_counters c;
    check(itm_get_counters(engine.GetScene()->handle, engine.GetRenderState()->handle, &c, nullptr), "counters");
    const size_t nPts = q.hd[3] == 0 ? (size_t)c.noTotalPoints : (size_t)P;
    check(itm_memcpy_d2h(pts.data(), ts->pointCloud_locations, nPts * 16, nullptr), "d2h");
    check(itm_memcpy_d2h(col.data(), ts->pointCloud_colours, nPts * 16, nullptr), "d2h");
    check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_RAYCAST_IMAGE, live.data(), live.size(), nullptr), "download");
    ids.resize((size_t)c.noVisibleEntries);
    if (c.noVisibleEntries) check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_VISIBLE_IDS, ids.data(), ids.size() * 4, nullptr), "download");
    std::vector<float> range(itm_buffer_bytes(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_RANGE_IMAGE) / 4);
    check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_RANGE_IMAGE, range.data(), range.size() * 4, nullptr), "download");
    const int32_t nv = c.noVisibleEntries;
    printf("{\"k\": %d, \"age\": %d, \"full\": %d, \"pose\": [", k, ts->age_pointCloud, ts->requiresFullRendering ? 1 : 0);
    for (int i = 0; i < 16; ++i) printf("%s%.9g", i ? ", " : "", ts->pose_d.GetM()[i]);
    printf("], \"digest\": [\"%016llx\", \"%016llx\", \"%016llx\", \"%016llx\", \"%016llx\"], \"visible\": %d, \"lastFreeBlockId\": %d}\n",
           (unsigned long long)fnv(pts.data(), nPts * 16), (unsigned long long)fnv(col.data(), nPts * 16), (unsigned long long)fnv(live.data(), live.size()),
           (unsigned long long)fnv(ids.data(), ids.size() * 4, fnv(&nv, 4)), (unsigned long long)fnv(range.data(), range.size() * 4), nv, c.lastFreeBlockId);
  }

  if (q.hd[15]) {      // the scene itself: table (hash scenes) and voxel blocks
    uint64_t d[2] = {0, 0};
    const int which[2] = {ITM_BUF_HASH_ENTRIES, ITM_BUF_VOXEL_BLOCKS};
    for (int i = 0; i < 2; ++i) {
      const size_t n = itm_buffer_bytes(engine.GetScene()->handle, nullptr, which[i]);
      if (!n) continue;
      std::vector<uint8_t> buf(n);
      check(itm_download(engine.GetScene()->handle, nullptr, which[i], buf.data(), n, nullptr), "download");
      d[i] = fnv(buf.data(), n);
    }
    printf("{\"scene_digest\": [\"%016llx\", \"%016llx\"]}\n", (unsigned long long)d[0], (unsigned long long)d[1]);
  }

  // what the images are compared with: the view's depth (and uncertainty) image, the live ray-cast image, the rgb input
  {
    const ITMView* view = engine.GetView();
    std::vector<float> depth((size_t)P);
    check(itm_memcpy_d2h(depth.data(), view->depth, (size_t)P * 4, nullptr), "d2h");
    check(itm_stream_synchronize(nullptr), "sync");
    dump(out, "view_depth.bin", depth.data(), depth.size() * 4);
    if (view->depthUncertainty) {
      check(itm_memcpy_d2h(depth.data(), view->depthUncertainty, (size_t)P * 4, nullptr), "d2h");
      check(itm_stream_synchronize(nullptr), "sync");
      dump(out, "view_uncertainty.bin", depth.data(), depth.size() * 4);
    }
    check(itm_download(engine.GetScene()->handle, engine.GetRenderState()->handle, ITM_BUF_RAYCAST_IMAGE, live.data(), live.size(), nullptr), "download");
    dump(out, "live_raycast_image.bin", live.data(), live.size());
    dump(out, "rgb_input.bin", rgb.data(), rgb.size());
    printf("{\"image_size\": [%d, %d]}\n", engine.GetImageSize().x, engine.GetImageSize().y);
  }

  auto report = [&](int t, const char* tag, Vector2i size, const ITMIntrinsics* intr) {
    ITMUChar4Image img(size);
    img.Clear(0x77);                                                 // GetImage clears it itself
    engine.GetImage(&img, (typename Engine::GetImageType)t, &freePose, intr);
    // the same image left on the device
    Vector2i ds;
    const uint8_t* dev = engine.GetImageDevice(&ds, (typename Engine::GetImageType)t, &freePose, intr, size);
    int deviceEqual = -1;
    if (dev) {
      std::vector<uint8_t> copy((size_t)ds.x * ds.y * 4);
      check(itm_memcpy_d2h(copy.data(), dev, copy.size(), nullptr), "d2h");
      check(itm_stream_synchronize(nullptr), "sync");
      deviceEqual = ds.x == img.noDims.x && ds.y == img.noDims.y && memcmp(copy.data(), img.GetData(), copy.size()) == 0 ? 1 : 0;
    }
    const std::string name = std::string(kTypeNames[t]) + tag;
    dump(out, (name + ".bin").c_str(), img.GetData(), img.dataSize * 4);
    printf("{\"image\": \"%s\", \"w\": %d, \"h\": %d, \"sha256\": \"%s\", \"device_equal\": %d}\n", name.c_str(), img.noDims.x, img.noDims.y,
           sha256(img.GetData(), img.dataSize * 4).c_str(), deviceEqual);
  };
  for (int t = 0; t < 7; ++t) {
    if (t == Engine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME && !colourVoxels) continue;
    report(t, "", freeSize, &freeIntr);
  }
  // a second free-camera call at another size: the free-view state follows the size
  if (freeSize2.x > 0) {
    report(Engine::InfiniTAM_IMAGE_FREECAMERA_SHADED, "_second_size", freeSize2, &freeIntr2);
    report(Engine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL, "_first_size_again", freeSize, &freeIntr);
  }
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  if (hRaw) { engine.GetViewBuilder()->WaitHostFramesRead(); }
  fflush(stdout);
  return 0;
}

static int bench(int calls) {
  // the bench scene of main_engine_demo: sphere of radius 0.5 m at (0, 0, 1.5) in front of a wall at 2.5 m, triangle-wave trajectory
  typedef ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> Engine;
  const int W = 640, H = 480, P = W * H, frames = 20;
  std::vector<int16_t> raw((size_t)frames * P);
  auto tri = [](int k) { return std::abs(((k + 25) % 100) - 50) - 25; };
  for (int k = 0; k < frames; ++k) {
    const float tx = 0.004f * (float)tri(k), ty = 0.002f * (float)tri(2 * k);
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
      const float dx = ((float)x - 320.f) / 580.f, dy = ((float)y - 240.f) / 580.f, ox = tx, oy = ty, oz = -1.5f;
      const float A = dx * dx + dy * dy + 1.f, B = 2.f * (ox * dx + oy * dy + oz), C = ox * ox + oy * oy + oz * oz - 0.25f, disc = B * B - 4.f * A * C;
      float z = 2.5f;
      if (disc > 0) { const float t = (-B - std::sqrt(disc)) / (2.f * A); if (t > 0) z = t; }
      raw[(size_t)k * P + y * W + x] = (int16_t)(z * 1000.f);
    }
  }
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, raw.size() * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  check(itm_memcpy_h2d(dRaw, raw.data(), raw.size() * 2, nullptr), "h2d");
  ITMLibSettings st; st.trackerType = ITMLibSettings::TRACKER_ICP;
  ITMSceneParams params(0.02f, 100, 0.004f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  Engine engine(st, params, calib, Vector2i{W, H}, Vector2i{W, H}, 1, 0.001f, 0.0f, 0x40000);
  for (int k = 0; k < frames; ++k) engine.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw + (size_t)k * P);
  check(itm_stream_synchronize(nullptr), "sync");
  ITMPose pose;
  float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.1f, -0.05f, 0.2f, 1};
  pose.SetM(M);
  ITMIntrinsics intr;
  printf("{\"calls_per_window\": %d, \"windows\": 9, \"get_image_device_us\": {", calls);
  bool first = true;
  for (int t = 0; t < 6; ++t) {
    if (t == Engine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME) continue;      // ITMVoxel_s stores no colour
    Vector2i size;
    for (int i = 0; i < 5; ++i) engine.GetImageDevice(&size, (Engine::GetImageType)t, &pose, &intr, Vector2i{W, H});
    check(itm_stream_synchronize(nullptr), "sync");
    std::vector<double> us;
    for (int w = 0; w < 9; ++w) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < calls; ++i) engine.GetImageDevice(&size, (Engine::GetImageType)t, &pose, &intr, Vector2i{W, H});
      check(itm_stream_synchronize(nullptr), "sync");
      us.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6 / calls);
    }
    std::sort(us.begin(), us.end());
    printf("%s\"%s\": {\"median\": %.2f, \"min\": %.2f, \"max\": %.2f}", first ? "" : ", ", kTypeNames[t], us[4], us[0], us[8]);
    first = false;
  }
  printf("}}\n");
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "--bench")) {
    try { return bench(atoi(argv[2])); } catch (const std::exception& e) { fprintf(stderr, "get_image_demo: %s\n", e.what()); return 1; }
  }
  if (argc < 3) { fprintf(stderr, "usage: %s <sequence file> <out dir>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Sequence q;
  if (!rd(f, q.hd, 16) || !rd(f, q.intr, 4) || !rd(f, q.freePose, 16) || !rd(f, q.freeIntr, 4) || !rd(f, q.freeIntr2, 4)) return 2;
  const size_t N = (size_t)q.hd[2], P = (size_t)q.hd[0] * q.hd[1];
  q.raw.resize(N * P); q.poses.resize(N * 16); q.fusion.resize(N); q.mainOn.resize(N);
  if (!rd(f, q.raw.data(), q.raw.size()) || (q.hd[6] && !rd(f, q.poses.data(), q.poses.size())) || !rd(f, q.fusion.data(), N) || !rd(f, q.mainOn.data(), N)) return 2;
  fclose(f);
  const std::string out = argv[2];
  try {
    if (q.hd[7] == 0 && q.hd[8] == 0) return run<ITMVoxel_s, ITMVoxelBlockHash>(q, out);
    if (q.hd[7] == 0 && q.hd[8] == 1) return run<ITMVoxel_s, ITMPlainVoxelArray>(q, out);
    if (q.hd[7] == 3 && q.hd[8] == 0) return run<ITMVoxel_f_rgb, ITMVoxelBlockHash>(q, out);
    if (q.hd[7] == 3 && q.hd[8] == 1) return run<ITMVoxel_f_rgb, ITMPlainVoxelArray>(q, out);
  } catch (const std::exception& e) {
    fprintf(stderr, "get_image_demo: %s\n", e.what());
    return 1;
  }
  fprintf(stderr, "unsupported voxel / index type\n");
  return 2;
}
