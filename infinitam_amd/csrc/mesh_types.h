// mesh_types.h -- the mesh handle shared by meshing.hip (triangles) and mesh_attributes.hip (per-vertex normals and colours).
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
};

namespace itm {

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
