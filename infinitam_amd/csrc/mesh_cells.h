// mesh_cells.h -- the two launches that turn a LIST of voxel blocks into triangles, as the full mesher (meshing.hip: the list of all
// allocated slots) and the incremental one (mesh_update.hip: the list of the dirty slots) both use them: one copy of the staging.
//   mesh_cells_kernel<COUNT>   one 512-lane workgroup per listed block.  The 9x9x9 SDF samples the block's cells touch (its own 8^3
//                              voxels plus one layer from the 7 neighbouring blocks, found through the block directory) are staged in LDS
//                              once; every lane classifies its cell from LDS (mc_device.h) and a workgroup scan gives the block's total.
//   mesh_scan_kernel           exclusive scan of per-block totals by one workgroup.
//   mesh_cells_kernel<WRITE>   the same staging, then every lane interpolates its cell's vertices with the reference's float operations
//                              and writes its triangles at base(block) + offset(cell), i.e. in the reference's order.
#pragma once

#include "itm_internal.h"
#include "mc_device.h"
#include "ordered_device.h"
#include "volume_device.h"
#include "wave_utils.h"

namespace itm {

// list[0 .. listCount->noVisibleEntries): table slots that hold a block (ptr >= 0).  COUNT: blockTriangles[b] = the triangles of listed
// block b.  WRITE: blockTriangles[b] = where its run starts among the totals[0] triangles of the whole mesh.
template <class VX, bool WRITE>
__global__ void __launch_bounds__(512) mesh_cells_kernel(VolumeView vol, const int32_t* __restrict__ list, const RenderCounters* __restrict__ listCount,
                                                         int32_t* __restrict__ blockTriangles, float* __restrict__ triangles, uint32_t maxTriangles,
                                                         const uint32_t* __restrict__ totals, float factor) {
  __shared__ float sdf[9 * 9 * 9];          // SDF_valueToFloat of the samples; NaN marks "no voxel stored there"
  __shared__ int nbBase[8];
  __shared__ int scan[9];
  const int nBlocks = listCount->noVisibleEntries;
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < nBlocks; b += gridDim.x) {
    const HashEntry he = unpack_entry(vol.hash[list[b]]);
    __syncthreads();                          // previous block's LDS contents are no longer needed
    if (t < 8) nbBase[t] = (t == 0) ? he.ptr * kBlockVoxels : block_base(vol, he.px + (t & 1), he.py + ((t >> 1) & 1), he.pz + (t >> 2));
    __syncthreads();
    for (int i = t; i < 729; i += 512) {
      const int x = i % 9, y = (i / 9) % 9, z = i / 81;
      const int base = nbBase[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
      float v = __builtin_nanf("");
      if (base >= 0) v = VX::to_float(VX::load_raw_sdf(vol.vba, (size_t)(base + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6))));
      sdf[i] = v;
    }
    __syncthreads();
    const int x = t & 7, y = (t >> 3) & 7, z = t >> 6;       // the reference's loop order: z outer, x inner == ascending t
    const McCell cell = classify_cell(sdf, x, y, z);
    int total;
    const int offset = block_exclusive_scan<8>(cell.nTri, scan, &total);
    if (!WRITE) {
      if (t == 0) blockTriangles[b] = total;
      continue;
    }
    if (cell.nTri == 0) continue;
    emit_cell(cell, he.px * kBlockSide + x, he.py * kBlockSide + y, he.pz * kBlockSide + z, (uint64_t)(uint32_t)blockTriangles[b] + (uint64_t)offset, totals[0],
              maxTriangles, factor, triangles);
  }
}

// exclusive scan of the per-block triangle counts (in place) by one workgroup; totals[0] = sum, totals[1] = count after the cap
static __global__ void __launch_bounds__(1024) mesh_scan_kernel(int32_t* __restrict__ blockTriangles, const RenderCounters* __restrict__ listCount,
                                                                uint32_t* __restrict__ totals, uint32_t maxTriangles) {
  // (prefixes < 2^32: at most 5 * 512 triangles per block, 2^18 blocks)
  const unsigned long long generated = carry_scan<16, unsigned long long>(
      listCount->noVisibleEntries, [&](int i) { return blockTriangles[i]; }, [&](int i, unsigned long long before) { blockTriangles[i] = (int32_t)(uint32_t)before; });
  if (threadIdx.x == 0) store_triangle_totals(totals, generated, maxTriangles);
}

constexpr int kMeshCellsGrid = 256 * 4;     // workgroups of a mesh_cells_kernel launch: each strides over the list

}  // namespace itm
