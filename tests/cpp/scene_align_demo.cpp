// Drives ITMSceneAlignEngine_HIP::AlignScene (include/itm_hip_engines.hpp; itm_scene_band_samples + itm_aligner_align).
//   scene_align_demo DST_TABLE DST_BLOCKS SRC_TABLE SRC_BLOCKS m0 .. m15
//       two hash scenes of 1 cm voxels (mu 4 cm, ITMVoxel_s) are uploaded from the four files (raw ITMHashEntry / ITMVoxel_s arrays, as
//       itm_upload takes them: tests/test_scene_align.py writes its analytic room corner), the band voxels of src are registered
//       against dst from the coarse pose m (dstFromSrc, 16 floats column-major), and one JSON line is printed: the refined pose as the
//       bits of its 16 floats, the result, and the evaluation at the refined pose.  The test computes the same through the Python
//       binding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;

typedef ITMScene<ITMVoxel_s, ITMVoxelBlockHash> Scene;

static std::vector<char> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::vector<char> data;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
  fclose(f);
  return data;
}

static void upload(Scene* s, const char* table, const char* blocks) {
  ITMSceneReconstructionEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>().ResetScene(s);
  const std::vector<char> t = read_file(table), b = read_file(blocks);
  check(itm_upload(s->handle, nullptr, ITM_BUF_HASH_ENTRIES, t.data(), t.size(), nullptr), "upload (table)");
  check(itm_upload(s->handle, nullptr, ITM_BUF_VOXEL_BLOCKS, b.data(), b.size(), nullptr), "upload (voxels)");
}

static void print_floats(const char* name, const float* v, int n, bool bits) {
  printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) {
    uint32_t w;
    memcpy(&w, &v[i], 4);
    if (bits) printf("%s%u", i ? ", " : "", w);
    else printf("%s%.9g", i ? ", " : "", (double)v[i]);
  }
  printf("]");
}

int main(int argc, char** argv) {
  try {
    if (argc != 21) {
      fprintf(stderr, "usage: scene_align_demo DST_TABLE DST_BLOCKS SRC_TABLE SRC_BLOCKS m0 .. m15\n");
      return 2;
    }
    ITMSceneParams params(0.04f, 100, 0.01f, 0.35f, 3.0f, false);
    Scene dst(&params, 0x1000), src(&params, 0x1000);
    upload(&dst, argv[1], argv[2]);
    upload(&src, argv[3], argv[4]);
    float m[16];
    for (int i = 0; i < 16; ++i) m[i] = strtof(argv[5 + i], nullptr);
    Matrix4f pose(m);
    ITMSceneAlignEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash> aligner;
    const itm_align_config cfg = aligner.DefaultConfig(&params);
    const int32_t count = aligner.SetSamplesFromScene(&src, cfg);
    itm_align_result r;
    aligner.Align(&dst, pose, cfg, &r);
    itm_align_eval e;
    aligner.Evaluate(&dst, pose, cfg, &e);
    printf("{\"samples\": %d, ", count);
    print_floats("pose_bits", pose.m, 16, true);
    printf(", \"status\": %d, \"evaluations\": %d, \"noValid\": %d, \"initialCost\": %.17g, \"finalCost\": %.17g, \"conditioning\": %.17g, ", r.status, r.evaluations,
           r.noValid, r.initialCost, r.finalCost, r.conditioning);
    printf("\"eval_noValid\": %d, ", e.noValid);
    print_floats("eval_f_bits", &e.f, 1, true);
    printf(", ");
    print_floats("eval_nabla_bits", e.nabla, 6, true);
    printf("}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "scene_align_demo: %s\n", e.what());
    return 1;
  }
}
