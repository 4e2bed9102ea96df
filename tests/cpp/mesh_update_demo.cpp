// Keeps a mesh up to date while the map grows, through the C++ adapters (itm_mesh_touch / itm_mesh_update).
//   mesh_update_demo adapter <out.stl>
//       Frames of a corrugated wall are fused into an ITMVoxel_s scene like ITMMainEngine::ProcessFrame does, the camera moving along x.
//       The scene is meshed after the first frame (ITMMeshingEngine_HIP::MeshScene); after every later frame the blocks it wrote are
//       marked (ITMMesh::Touch with the frame's render state) and the mesh is updated (ITMMeshingEngine_HIP::UpdateMesh).  The mesh is
//       written as binary STL; tests/test_mesh_update.py builds the same scene through the Python binding and compares the files.
//   mesh_update_demo engine <live.stl> <export.stl>
//       ITMMainEngine_HIP with settings.liveMeshEveryNFrames = 2 over six frames with poses from outside: its live mesh, and the mesh
//       SaveSceneToMesh makes from scratch, as binary STL -- the same bytes.
// Prints the statistics of the last update as JSON.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "itm_hip_engines.hpp"

using namespace itmhip;
typedef ITMVoxel_s V;
typedef ITMVoxelBlockHash I;

static const int W = 160, H = 120, P = W * H;

static void print_stats(const itm_mesh_update_stats& s, uint32_t noChanged, uint32_t noRemoved) {
  printf("{\"full\": %d, \"allocated\": %d, \"marked\": %d, \"ignoredMarks\": %d, \"appeared\": %d, \"vanished\": %d, \"remeshed\": %d, \"kept\": %d, "
         "\"trianglesBefore\": %u, \"trianglesAfter\": %u, \"trianglesCopied\": %u, \"trianglesGenerated\": %u, \"noChanged\": %u, \"noRemoved\": %u}\n",
         s.full, s.allocated, s.marked, s.ignoredMarks, s.appeared, s.vanished, s.remeshed, s.kept, s.trianglesBefore, s.trianglesAfter, s.trianglesCopied,
         s.trianglesGenerated, noChanged, noRemoved);
}

static int adapter(const char* out) {
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMScene<V, I> scene(&params);
  ITMDenseMapper_HIP<V, I> mapper;
  ITMVisualisationEngine_HIP<V, I> vis(&scene);
  ITMTrackingController_HIP<V, I> controller(&vis);
  mapper.ResetScene(&scene);
  ITMRenderState* rs = vis.CreateRenderState(Vector2i{W, H});
  std::vector<float> depth(P);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) depth[x + y * W] = 1.5f + 0.002f * (float)((x * 7 + y * 13) % 50);
  void *dDepth, *dPts, *dNrm;
  check(itm_dev_malloc(&dDepth, P * 4), "malloc"); check(itm_dev_malloc(&dPts, P * 16), "malloc"); check(itm_dev_malloc(&dNrm, P * 16), "malloc");
  check(itm_memcpy_h2d(dDepth, depth.data(), P * 4, nullptr), "h2d");
  ITMView view;
  view.calib.intrinsics_d.SetFrom(145.f, 145.f, 80.f, 60.f);
  view.calib.intrinsics_rgb = view.calib.intrinsics_d;
  view.depth = (const float*)dDepth;
  view.depthSize = Vector2i{W, H}; view.rgbSize = Vector2i{W, H};
  ITMTrackingState ts;
  ts.pointCloud_locations = (float*)dPts; ts.pointCloud_colours = (float*)dNrm;

  ITMMesh mesh(&scene);
  ITMMeshingEngine_HIP<V, I> mesher;
  itm_mesh_update_stats stats;
  memset(&stats, 0, sizeof stats);
  for (int k = 0; k < 3; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.2f * k, 0, 0, 1};
    ts.pose_d.SetM(M);
    controller.Track(&ts, &view);
    mapper.ProcessFrame(&view, &ts, &scene, rs);
    controller.Prepare(&ts, &view, rs);
    if (k == 0) { mesher.MeshScene(&mesh, &scene); continue; }
    mesh.Touch(&scene, rs);
    stats = mesher.UpdateMesh(&mesh, &scene);
  }
  std::vector<itm_mesh_changed_block> changed;
  std::vector<itm_mesh_removed_block> removed;
  mesh.DownloadUpdate(changed, removed);
  if (mesh.noTotalTriangles != stats.trianglesAfter) throw std::runtime_error("the adapter's count is not the update's");
  mesh.WriteSTL(out);
  print_stats(stats, (uint32_t)changed.size(), (uint32_t)removed.size());
  delete rs;
  itm_dev_free(dDepth); itm_dev_free(dPts); itm_dev_free(dNrm);
  return 0;
}

static int engine(const char* live, const char* exported) {
  typedef ITMMainEngine_HIP<V, I> Engine;
  ITMLibSettings st;
  st.trackerType = ITMLibSettings::TRACKER_EXTERNAL;
  st.liveMeshEveryNFrames = 2;
  ITMSceneParams params(0.02f, 100, 0.01f, 0.35f, 3.0f, false);
  ITMRGBDCalib calib;
  calib.intrinsics_d.SetFrom(145.0f, 145.0f, 80.0f, 60.0f);
  calib.intrinsics_rgb = calib.intrinsics_d;
  Engine e(st, params, calib, Vector2i{W, H}, Vector2i{W, H});
  std::vector<int16_t> raw(P);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) raw[x + y * W] = (int16_t)(1500 + 2 * ((x * 7 + y * 13) % 50));      // millimetres
  void *dRaw, *dRgb;
  check(itm_dev_malloc(&dRaw, (size_t)P * 2), "malloc"); check(itm_dev_malloc(&dRgb, (size_t)P * 4), "malloc");
  check(itm_memcpy_h2d(dRaw, raw.data(), (size_t)P * 2, nullptr), "h2d");
  check(itm_stream_synchronize(nullptr), "sync");
  int updates = 0;
  for (int k = 0; k < 6; ++k) {
    float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.2f * k, 0, 0, 1};
    e.GetTrackingState()->pose_d.SetM(M);
    e.ProcessFrame((const uint8_t*)dRgb, (const int16_t*)dRaw);
    if (k % 2 == 1) {
      const itm_mesh_update_stats& s = e.GetLastMeshUpdateStats();
      if (s.allocated <= 0 || (k > 1 && s.full != 0)) throw std::runtime_error("the live mesh was not updated after an even number of frames");
      ++updates;
    }
  }
  if (!e.GetLiveMesh() || updates != 3) throw std::runtime_error("no live mesh");
  check(itm_mesh_write_stl(e.GetLiveMesh(), live, nullptr), "write the live mesh");
  e.SaveSceneToMesh(exported);
  const itm_mesh_update_stats s = e.GetLastMeshUpdateStats();
  print_stats(s, s.noChanged, s.noRemoved);
  itm_dev_free(dRaw); itm_dev_free(dRgb);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 3 && !strcmp(argv[1], "adapter")) return adapter(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "engine")) return engine(argv[2], argv[3]);
    fprintf(stderr, "usage: %s adapter <out.stl> | engine <live.stl> <export.stl>\n", argv[0]);
    return 2;
  } catch (const std::exception& ex) {
    fprintf(stderr, "mesh_update_demo: %s\n", ex.what());
    return 1;
  }
}
