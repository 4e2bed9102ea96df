// mesh_types.h -- the mesh handle shared by meshing.hip (triangles), mesh_attributes.hip (per-vertex normals and colours) and
// mesh_index.hip (the indexed form: shared vertices and faces).
#pragma once

#include <mutex>

#include "itm_internal.h"
#include "mc_tables.h"
#include "shading_device.h"

struct itm_mesh {
  const itm_scene* scene = nullptr;
  uint32_t maxTriangles = 0;
  itm::DeviceBuffer<float> triangles;        // ITMMesh::Triangle[maxTriangles]: 9 floats (p0, p1, p2)
  itm::DeviceBuffer<int32_t> slots;          // allocated slots in ascending order
  itm::DeviceBuffer<int32_t> blockTriangles; // per listed block: triangle count, then exclusive prefix
  itm::DeviceBuffer<uint8_t> flags;          // per slot: allocated?
  itm::DeviceBuffer<int32_t> chunkCount;
  itm::DeviceBuffer<itm::RenderCounters> listCounters;   // noVisibleEntries = number of listed blocks
  itm::DeviceBuffer<uint32_t> totals;        // [0] triangles generated, [1] noTotalTriangles (after the cap)
  int capBlocks = 0;
  // itm_mesh_volume on a dense scene (mesh_dense.hip); allocated by the first such call
  itm::DeviceBuffer<int32_t> brickCount;     // per 8^3 brick of the array: triangle count
  itm::DeviceBuffer<unsigned long long> brickBase;   // per brick: triangles generated before it
  itm::DeviceBuffer<int32_t> brickList;      // the bricks that have triangles, ascending
  itm::DeviceBuffer<int32_t> brickCounters;  // [0] number of listed bricks; [2..3] triangles generated (64 bits)
  bool fromVolume = false;           // the buffer holds the mesh itm_mesh_volume made of a dense scene; itm_mesh_scene clears it
  // vertex attributes of the triangles the last itm_mesh_scene left in the buffer (mesh_attributes.hip); allocated on first use
  itm::DeviceBuffer<float> normals;          // 3 floats per vertex, 3 vertices per triangle, buffer order
  itm::DeviceBuffer<uchar4> colours;         // one per vertex
  uint32_t attrCurrent = 0;          // ITM_MESH_* bits computed for the buffer's present contents; itm_mesh_scene clears it
  // indexed form of the buffer's present contents (mesh_index.hip); allocated / grown by itm_mesh_index, sized from the counts
  itm::DeviceBuffer<float> vertices;         // 3 floats per unique vertex, in the order of first occurrence in the buffer
  itm::DeviceBuffer<uint32_t> faces;         // 3 vertex indices per triangle, buffer order
  itm::DeviceBuffer<uint32_t> first;         // per unique vertex: the smallest soup vertex index that holds its position (strictly ascending)
  itm::DeviceBuffer<uint32_t> rep;           // per soup vertex: first[] of its position (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexTable;    // the hash set of representatives (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexChunks;   // per chunk of soup vertices: unique vertices first seen there, then exclusive prefix, closed by nV
  itm::DeviceBuffer<int32_t> blockVertex;    // per listed block: its first unique vertex (the vertices first seen in block b are [b], [b + 1])
  uint32_t noVertices = 0, noIndexedTriangles = 0;
  bool indexCurrent = false;         // the index describes the buffer's present contents; itm_mesh_scene clears it
  // attributes of the unique vertices (itm_mesh_indexed_attributes), independent of the soup's
  itm::DeviceBuffer<float> vertexNormals;    // 3 floats per unique vertex
  itm::DeviceBuffer<uchar4> vertexColours;   // one per unique vertex
  uint32_t indexedAttrCurrent = 0;   // ITM_MESH_* bits computed for the present index; itm_mesh_scene and itm_mesh_index clear it
};

namespace itm {

int launch_mesh_volume_dense(const itm_scene* s, itm_mesh* m, hipStream_t st);   // mesh_dense.hip

// ---- the per-cell pieces the hash mesher (meshing.hip) and the dense mesher (mesh_dense.hip) share: one copy, so the two cannot drift ----

// which of the 12 edges a sign configuration crosses: an edge is crossed when its two corners have different signs
__device__ inline uint32_t crossed_edges(uint32_t cube) {
  uint32_t mask = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e)
    if (((cube >> kCubeEdge[e][0]) ^ (cube >> kCubeEdge[e][1])) & 1u) mask |= 1u << e;
  return mask;
}

// sdfInterp (DeviceAgnostic/ITMMeshingEngine.h:194-201), per component; p1/p2 are integer-valued voxel coordinates
__device__ inline void edge_vertex(const float* p1, const float* p2, float v1, float v2, float* out) {
  if (fabsf(0.0f - v1) < 0.00001f) { out[0] = p1[0]; out[1] = p1[1]; out[2] = p1[2]; return; }
  if (fabsf(0.0f - v2) < 0.00001f) { out[0] = p2[0]; out[1] = p2[1]; out[2] = p2[2]; return; }
  if (fabsf(v1 - v2) < 0.00001f) { out[0] = p1[0]; out[1] = p1[1]; out[2] = p1[2]; return; }
  const float t = (0.0f - v1) / (v2 - v1);
  out[0] = p1[0] + t * (p2[0] - p1[0]);
  out[1] = p1[1] + t * (p2[1] - p1[1]);
  out[2] = p1[2] + t * (p2[2] - p1[2]);
}

// what a mesher's scan leaves in itm_mesh::totals: [0] = the triangles generated, [1] = noTotalTriangles -- the reference's count stops at
// noMaxTriangles - 1 (its last slot keeps being overwritten, _CPU.cpp:48-52)
__device__ inline void store_triangle_totals(uint32_t* totals, unsigned long long generated, uint32_t maxTriangles) {
  totals[0] = (uint32_t)generated;
  totals[1] = (generated < (unsigned long long)maxTriangles - 1ull) ? (uint32_t)generated : maxTriangles - 1u;
}

// kTriangleCases into a translation unit's constant-memory table (a constant symbol belongs to its code object, so each mesher has
// its own; TAG keeps their "done" flags apart): once per device, also when several host threads create meshes at the same time
template <class TAG>
inline int upload_case_table(const void* symbol) {
  static std::mutex guard;
  static bool done[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lock(guard);
  if (!done[dev]) {
    ITM_HIP(hipMemcpyToSymbol(symbol, kTriangleCases, sizeof(kTriangleCases)));
    done[dev] = true;
  }
  return ITM_OK;
}

// block base (voxel index of its first voxel) of block (bx, by, bz), or -1: directory where it covers, table walk elsewhere
__device__ inline int block_base(const VolumeView& vol, int bx, int by, int bz) {
  const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
  if (vol.dirPtr && dir_covers(ux, uy, uz)) {
    const int ptr = vol.dirPtr[dir_cell(ux, uy, uz)];
    return ptr < 0 ? -1 : ptr * kBlockVoxels;
  }
  if ((int)(int16_t)bx != bx || (int)(int16_t)by != by || (int)(int16_t)bz != bz) return -1;   // beyond the table's short coordinates
  return resolve_block(vol, unpack_entry(vol.hash[hash_index(bx, by, bz, vol.mask)]), bx, by, bz);
}

}  // namespace itm
