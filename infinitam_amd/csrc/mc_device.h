// mc_device.h -- one marching-cubes cell, as the hash mesher (meshing.hip) and the dense mesher (mesh_dense.hip) both state it: one copy,
// so the two cannot drift.  The kernels stage the 9^3 samples of a block or brick and scan the counts their own way; what happens to a
// cell between the staged samples and its triangles in the buffer is here.
//
// Reference behaviour restated:
//   findPointNeighbors / sdfInterp / buildVertList   DeviceAgnostic/ITMMeshingEngine.h:153-231
//   the full buffer (last slot overwritten)          DeviceSpecific/CPU/ITMMeshingEngine_CPU.cpp:48-52
#pragma once

#include "mc_tables.h"

namespace itm {

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

struct McCell {
  float val[8];      // sdf at the corners, in kCubeCorner order
  uint32_t cube;     // sign configuration: bit k set <=> corner k negative
  uint64_t list;     // kTriangleCases[cube]; empty for a cell that makes no triangle
  int nTri;
};

// Cell (x, y, z) of the staged samples sdf[x + 9 y + 81 z] (SDF_valueToFloat of the voxels; NaN marks "no voxel stored there")
__device__ inline McCell classify_cell(const float* sdf, int x, int y, int z) {
  McCell c;
  bool ok = true;
  c.cube = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = kCubeCorner[k];
    c.val[k] = sdf[(x + (o & 1)) + (y + ((o >> 1) & 1)) * 9 + (z + (o >> 2)) * 81];
    ok = ok && !(c.val[k] != c.val[k]) && !(c.val[k] == 1.0f);   // findPointNeighbors: every corner stored and != 1.0f
    if (c.val[k] < 0.0f) c.cube |= 1u << k;
  }
  c.nTri = 0;
  c.list = ~0ull;
  if (ok && c.cube != 0u && c.cube != 255u) {
    c.list = kTriangleCases[c.cube];
    for (uint64_t l = c.list; (l & 0xfull) != 0xfull; l >>= 12) ++c.nTri;
  }
  return c;
}

// The triangles of a classified cell whose first corner is the voxel (lx, ly, lz) (global voxel coordinates), written as triangles g,
// g + 1, ... of the `generated` the whole mesh has: vertices on the crossed edges in voxel units, scaled by `factor` (the voxel size)
__device__ inline void emit_cell(const McCell& c, int lx, int ly, int lz, uint64_t g, uint64_t generated, uint32_t maxTriangles, float factor,
                                 float* __restrict__ triangles) {
  float corner[8][3];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int o = kCubeCorner[k];
    // (blockLocation + offset).toFloat(): integer sum converted, the same value as the float sum for these magnitudes
    corner[k][0] = (float)(lx + (o & 1)); corner[k][1] = (float)(ly + ((o >> 1) & 1)); corner[k][2] = (float)(lz + (o >> 2));
  }
  const uint32_t edges = crossed_edges(c.cube);
  float vert[12][3];
#pragma unroll
  for (int e = 0; e < 12; ++e)
    if (edges & (1u << e)) edge_vertex(corner[kCubeEdge[e][0]], corner[kCubeEdge[e][1]], c.val[kCubeEdge[e][0]], c.val[kCubeEdge[e][1]], vert[e]);
  for (uint64_t l = c.list; (l & 0xfull) != 0xfull; l >>= 12, ++g) {
    // triangles[noTriangles] = ...; if (noTriangles < noMaxTriangles - 1) noTriangles++   (_CPU.cpp:48-52)
    uint64_t dst = g;
    if (g >= (uint64_t)maxTriangles - 1ull) {
      if (g != generated - 1ull) continue;            // only the last triangle generated survives in the last slot
      dst = (uint64_t)maxTriangles - 1ull;
    }
    float* o = triangles + dst * 9ull;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = (int)((l >> (4 * k)) & 0xfull);
      // a dynamically indexed private array would live in scratch: select through a switch-free chain over the 12 edges
      float vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll
      for (int q = 0; q < 12; ++q) if (q == e) { vx = vert[q][0]; vy = vert[q][1]; vz = vert[q][2]; }
      o[3 * k + 0] = vx * factor; o[3 * k + 1] = vy * factor; o[3 * k + 2] = vz * factor;
    }
  }
}

}  // namespace itm
