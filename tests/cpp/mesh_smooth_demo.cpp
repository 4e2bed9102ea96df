// Exports a smoothed mesh through the C++ adapter: two frames of a corrugated wall with a colour pattern are fused into an
// ITMVoxel_s_rgb scene like ITMMainEngine::ProcessFrame does, the scene is meshed (ITMMeshingEngine_HIP), welded into shared vertices
// (ITMMesh::Index), smoothed in fixed point (ITMMesh::Smooth: 20 Taubin passes, border vertices pinned), the normals and colours of the
// unique vertices are read at the smoothed positions (ITMMesh::ComputeIndexedAttributes) and the indexed mesh is written as a binary PLY.
//   mesh_smooth_demo <out.ply>
// Prints the counts as JSON; tests/test_mesh_smooth.py builds the same scene through the Python binding and compares the files.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s_rgb V;
typedef ITMVoxelBlockHash I;

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <out.ply>\n", argv[0]); return 2; }
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
  ITMMesh mesh(&scene);
  ITMMeshingEngine_HIP<V, I> mesher;
  mesher.MeshScene(&mesh, &scene);
  mesh.Index();
  const itm_mesh_smooth_stats stats = mesh.Smooth();
  mesh.ComputeIndexedAttributes(&scene, ITM_MESH_NORMALS | ITM_MESH_COLOURS);
  mesh.WriteIndexedPLY(argv[1]);
  printf("{\"triangles\": %u, \"vertices\": %u, \"moving\": %u, \"irregular\": %u, \"isolated\": %u, \"max_entries\": %u, \"steps\": %u}\n",
         mesh.noTotalTriangles, stats.noVertices, stats.noMoving, stats.noIrregular, stats.noIsolated, stats.maxEntries, stats.steps);
  delete rs;
  itm_dev_free(dDepth); itm_dev_free(dRgb); itm_dev_free(dPts); itm_dev_free(dNrm);
  return 0;
}
