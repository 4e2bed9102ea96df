// meshing.hip -- marching-cubes mesh of the hash scene.
//
// Reference behaviour:
//   ITMMeshingEngine_CPU<TVoxel, ITMVoxelBlockHash>::MeshScene   DeviceSpecific/CPU/ITMMeshingEngine_CPU.cpp:19-58
//   findPointNeighbors / sdfInterp / buildVertList               DeviceAgnostic/ITMMeshingEngine.h:153-231
//   ITMMesh (triangle buffer, noMaxTriangles, WriteOBJ, WriteSTL) Objects/ITMMesh.h:14-124
//   (ITMPlainVoxelArray: MeshScene is empty in the reference, :70-72 -> no triangles here either)
//
// The reference walks the table slot by slot, the 512 voxels of every allocated block in z, y, x order, and appends the
// triangles of each cell to one array -- so the array's ORDER is defined, and so is what happens when it is full (the last
// slot keeps being overwritten, the count stops at noMaxTriangles - 1).  Both are reproduced exactly:
//
// MI355X design: three launches over a device-resident list of the allocated slots (ordered compaction, as the visible list).
//   1. mesh_cells_kernel<COUNT>: one 512-lane workgroup per allocated block.  The 9x9x9 SDF samples the block's cells touch
//      (its own 8^3 voxels plus one layer from the 7 neighbouring blocks, found through the block directory) are staged in
//      LDS once; every lane then classifies its cell from LDS (sign configuration -> triangle count) and a workgroup scan
//      gives the block's total.
//   2. mesh_scan_kernel: exclusive scan of the per-block totals (one workgroup; meshing is an export step, not a frame step).
//   3. mesh_cells_kernel<WRITE>: the same staging, then every lane interpolates its cell's vertices with the reference's float
//      operations and writes its triangles at base(block) + offset(cell), i.e. in the reference's order.
// The kernels of 1-3 take any list of blocks and stand in mesh_cells.h: the frame step, itm_mesh_update (mesh_update.hip), runs them
// over the blocks a frame touched.  For it, a fourth launch here records which run of the buffer belongs to which block.
#include <new>

#include "itm_internal.h"
#include "mesh_cells.h"
#include "mesh_types.h"

namespace itm {

__global__ void __launch_bounds__(256) mesh_flag_kernel(const uint4* __restrict__ hash, int nEntries, uint8_t* __restrict__ flags, int32_t* __restrict__ chunkCount) {
  flag_chunk(nEntries, flags, chunkCount, [&](int slot) { return (int)hash[slot].w >= 0; });
}

// the soup on the host, with the attributes that are current where the writer carries them
int fetch_soup(const itm_mesh* m, bool withAttributes, FetchedMesh& out, itm_stream stream) {
  uint32_t n = 0;
  int rc = itm_mesh_info(m, &n, nullptr, nullptr, stream);
  if (rc) return rc;
  const uint32_t have = withAttributes ? m->attributes(false) : 0u;
  out.resize((size_t)n * 3, n, false, have & ITM_MESH_NORMALS, have & ITM_MESH_COLOURS);
  if ((rc = itm_mesh_download(m, out.positions.data(), n, &n, stream)) || !have) return rc;
  return itm_mesh_download_attributes(m, out.normals_or_null(), out.colours_or_null(), n, &n, stream);
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_create(const itm_scene* s, uint32_t maxTriangles, itm_mesh** out) {
  if (!s || !out) return set_error(ITM_ERR_INVALID, "null argument");
  itm_mesh* m = new (std::nothrow) itm_mesh();
  if (!m) return set_error(ITM_ERR_DEVICE, "out of host memory");
  m->scene = s;
  const bool hash = s->cfg.indexType == ITM_INDEX_HASH;
  m->maxTriangles = maxTriangles ? maxTriangles : (uint32_t)s->cfg.localBlockNum * 32u;   // ITMMesh::noMaxTriangles (Objects/ITMMesh.h:23)
  if (m->maxTriangles < 2) { delete m; return set_error(ITM_ERR_INVALID, "a mesh needs room for at least two triangles"); }
  m->capBlocks = hash ? s->cfg.localBlockNum : 0;
  hipError_t e = m->triangles.alloc((size_t)m->maxTriangles * 9);
  if (e == hipSuccess) e = m->totals.alloc(2);
  if (e == hipSuccess) e = hipMemset(m->totals, 0, 8);
  if (e == hipSuccess && hash) e = m->slots.alloc((size_t)m->capBlocks);
  if (e == hipSuccess && hash) e = m->blockTriangles.alloc((size_t)m->capBlocks);
  if (e == hipSuccess && hash) e = m->flags.alloc((size_t)s->numChunks * kSweepChunk);
  if (e == hipSuccess && hash) e = m->chunkCount.alloc((size_t)s->numChunks);
  if (e == hipSuccess && hash) e = m->listCounters.alloc(1);
  if (e == hipSuccess && hash) e = alloc_update_arena(s, m);
  if (e == hipSuccess) e = hipMemset(m->triangles, 0, (size_t)m->maxTriangles * 36);   // MemoryBlock storage starts zeroed
  if (e != hipSuccess) { delete m; return hip_fail(e, "mesh buffers", __FILE__, __LINE__); }
  *out = m;
  return ITM_OK;
}

int itm_mesh_destroy(itm_mesh* m) { delete m; return ITM_OK; }

int itm_mesh_scene(const itm_scene* s, itm_mesh* m, itm_stream stream) {
  if (!s || !m) return set_error(ITM_ERR_INVALID, "null argument");
  if (m->scene != s) return set_error(ITM_ERR_INVALID, "mesh belongs to another scene");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  m->soup_remeshed();                                          // attributes, index and components belong to the mesh that is being replaced
  // mesh->triangles->Clear()
  ITM_HIP(hipMemsetAsync(m->triangles, 0, (size_t)m->maxTriangles * 36, st));
  ITM_HIP(hipMemsetAsync(m->totals, 0, 8, st));
  if (s->cfg.indexType != ITM_INDEX_HASH) return ITM_OK;       // ITMPlainVoxelArray: empty in the reference
  mesh_flag_kernel<<<s->numChunks, 256, 0, st>>>(s->hash, s->noTotalEntries, m->flags, m->chunkCount);
  int rc = launch_ordered_compaction(m->flags.get(), m->chunkCount, s->numChunks, s->noTotalEntries, m->slots, m->capBlocks, &m->listCounters->rawVisibleCount,
                                      &m->listCounters->noVisibleEntries, st);
  if (rc) return rc;
  const VolumeView vol = make_volume(s);
  const int grid = kMeshCellsGrid;
  rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
    using VX = decltype(vx);
    mesh_cells_kernel<VX, false><<<grid, 512, 0, st>>>(vol, m->slots, m->listCounters, m->blockTriangles, m->triangles, m->maxTriangles, m->totals, s->prm.voxelSize);
    mesh_scan_kernel<<<1, 1024, 0, st>>>(m->blockTriangles, m->listCounters, m->totals, m->maxTriangles);
    mesh_cells_kernel<VX, true><<<grid, 512, 0, st>>>(vol, m->slots, m->listCounters, m->blockTriangles, m->triangles, m->maxTriangles, m->totals, s->prm.voxelSize);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  return record_run_table(s, m, st);                           // (the buffer and the counts are not touched)
}

// The mesh of the scene's volume whatever its index: a hash scene as itm_mesh_scene, a dense scene brick by brick (mesh_dense.hip)
int itm_mesh_volume(const itm_scene* s, itm_mesh* m, itm_stream stream) {
  if (!s || !m) return set_error(ITM_ERR_INVALID, "null argument");
  if (s->cfg.indexType == ITM_INDEX_HASH) return itm_mesh_scene(s, m, stream);
  const int rc = itm_mesh_scene(s, m, stream);                 // checks, recorded calls, stale marks, cleared buffer and totals
  if (rc) return rc;
  const int rv = launch_mesh_volume_dense(s, m, as_stream(stream));
  if (rv) return rv;
  m->meshed_from_volume();
  return ITM_OK;
}

int itm_mesh_info(const itm_mesh* m, uint32_t* noTotalTriangles, uint32_t* noMaxTriangles, const float** triangles_dev, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  uint32_t t[2] = {0, 0};
  hipStream_t st = as_stream(stream);
  ITM_HIP(hipMemcpyAsync(t, m->totals, 8, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (noTotalTriangles) *noTotalTriangles = t[1];
  if (noMaxTriangles) *noMaxTriangles = m->maxTriangles;
  if (triangles_dev) *triangles_dev = m->triangles;
  return ITM_OK;
}

int itm_mesh_download(const itm_mesh* m, float* dst_host, uint32_t capacityTriangles, uint32_t* noTotalTriangles, itm_stream stream) {
  if (!m || !noTotalTriangles) return set_error(ITM_ERR_INVALID, "null argument");
  int rc = itm_mesh_info(m, noTotalTriangles, nullptr, nullptr, stream);
  if (rc) return rc;
  if (*noTotalTriangles && capacityTriangles && !dst_host) return set_error(ITM_ERR_INVALID, "null destination");
  hipStream_t st = as_stream(stream);
  ITM_HIP(copy_out(dst_host, m->triangles, *noTotalTriangles, capacityTriangles, 36, st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

// ITMMesh::WriteOBJ and ITMMesh::WriteSTL of the triangle buffer (mesh_files.h)
int itm_mesh_write_obj(const itm_mesh* m, const char* path, itm_stream stream) {
  if (!m || !path) return set_error(ITM_ERR_INVALID, "null argument");
  FetchedMesh h;
  const int rc = fetch_soup(m, false, h, stream);
  return rc ? rc : file_status(write_obj(h.view, path));
}

int itm_mesh_write_stl(const itm_mesh* m, const char* path, itm_stream stream) {
  if (!m || !path) return set_error(ITM_ERR_INVALID, "null argument");
  FetchedMesh h;
  const int rc = fetch_soup(m, false, h, stream);
  return rc ? rc : file_status(write_stl(h.view, path));
}

}  // extern "C"
