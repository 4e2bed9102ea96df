// mesh_types.h -- the mesh handle shared by meshing.hip (triangles), mesh_attributes.hip (per-vertex normals and colours) and
// mesh_index.hip (the indexed form: shared vertices and faces).
#pragma once

#include "itm_internal.h"
#include "shading_device.h"

struct itm_mesh {
  const itm_scene* scene = nullptr;
  uint32_t maxTriangles = 0;
  float* triangles = nullptr;        // ITMMesh::Triangle[maxTriangles]: 9 floats (p0, p1, p2)
  int32_t* slots = nullptr;          // allocated slots in ascending order
  int32_t* blockTriangles = nullptr; // per listed block: triangle count, then exclusive prefix
  uint8_t* flags = nullptr;          // per slot: allocated?
  int32_t* chunkCount = nullptr;
  itm::RenderCounters* listCounters = nullptr;   // noVisibleEntries = number of listed blocks
  uint32_t* totals = nullptr;        // [0] triangles generated, [1] noTotalTriangles (after the cap)
  int capBlocks = 0;
  // vertex attributes of the triangles the last itm_mesh_scene left in the buffer (mesh_attributes.hip); allocated on first use
  float* normals = nullptr;          // 3 floats per vertex, 3 vertices per triangle, buffer order
  uchar4* colours = nullptr;         // one per vertex
  uint32_t attrCurrent = 0;          // ITM_MESH_* bits computed for the buffer's present contents; itm_mesh_scene clears it
  // indexed form of the buffer's present contents (mesh_index.hip); allocated / grown by itm_mesh_index, sized from the counts
  float* vertices = nullptr;         // 3 floats per unique vertex, in the order of first occurrence in the buffer
  uint32_t* faces = nullptr;         // 3 vertex indices per triangle, buffer order
  uint32_t* first = nullptr;         // per unique vertex: the smallest soup vertex index that holds its position (strictly ascending)
  uint32_t* rep = nullptr;           // per soup vertex: first[] of its position (scratch of the build)
  uint32_t* indexTable = nullptr;    // the hash set of representatives (scratch of the build)
  uint32_t* indexChunks = nullptr;   // per chunk of soup vertices: unique vertices first seen there, then exclusive prefix; [capIndexChunks] = nV
  int32_t* blockVertex = nullptr;    // per listed block: its first unique vertex (the vertices first seen in block b are [b], [b + 1])
  size_t capRep = 0, capFaces = 0, capFirst = 0, capVertices = 0, capIndexTable = 0, capIndexChunks = 0;   // in elements
  uint32_t noVertices = 0, noIndexedTriangles = 0;
  bool indexCurrent = false;         // the index describes the buffer's present contents; itm_mesh_scene clears it
  // attributes of the unique vertices (itm_mesh_indexed_attributes), independent of the soup's
  float* vertexNormals = nullptr;    // 3 floats per unique vertex
  uchar4* vertexColours = nullptr;   // one per unique vertex
  size_t capVertexNormals = 0, capVertexColours = 0;
  uint32_t indexedAttrCurrent = 0;   // ITM_MESH_* bits computed for the present index; itm_mesh_scene and itm_mesh_index clear it
};

namespace itm {

// (re)allocates *p for `need` elements of `elem` bytes when the present capacity is smaller; the old contents are not kept
inline int grow_device(void** p, size_t* cap, size_t need, size_t elem, const char* what) {
  if (need <= *cap) return ITM_OK;
  (void)hipFree(*p);
  *p = nullptr; *cap = 0;
  const hipError_t e = hipMalloc(p, need * elem);
  if (e != hipSuccess) { *p = nullptr; return hip_fail(e, what, __FILE__, __LINE__); }
  *cap = need;
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
