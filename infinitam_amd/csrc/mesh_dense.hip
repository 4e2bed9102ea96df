// mesh_dense.hip -- marching-cubes mesh of a dense scene (ITMPlainVoxelArray): itm_mesh_volume.
//
// The reference has no dense mesher (ITMMeshingEngine_CPU<TVoxel, ITMPlainVoxelArray>::MeshScene is empty, DeviceSpecific/CPU/
// ITMMeshingEngine_CPU.cpp:68-70; itm_mesh_scene keeps that).  This one is defined by the reference's own per-cell function:
//   * the array is cut into bricks of 8^3 voxels by array index, brick (bx, by, bz) = voxels 8b .. 8b + 7 clipped to the array;
//   * bricks are visited in ascending bx + by * nbx + bz * nbx * nby, the cells of a brick as `for z for y for x` (the loop of
//     _CPU.cpp:39 on one block);
//   * cell (x, y, z) is buildVertList (DeviceAgnostic/ITMMeshingEngine.h:204-232) at L = (x, y, z) + denseOffset, its corners read
//     through the dense readVoxel (ITMRepresentationAccess.h:129-142): a corner outside the array is "not found";
//   * the buffer is ITMMesh's: cleared first, the count stops at noMaxTriangles - 1, the last slot keeps the last triangle generated.
// A hash scene whose blocks hold the same voxels at the same global positions gives the same triangles, block run for block run --
// both kernels classify and emit a cell through mc_device.h.
//
// MI355X design: three launches, no host round trip.
//   1. mesh_bricks_kernel<COUNT>: persistent 512-lane workgroups stride over all bricks.  The 9^3 sdf samples of a brick (its voxels
//      and the +1 planes of its neighbours, NaN outside the array) go through registers into LDS: lane i loads sample i (x fastest,
//      so a wave reads whole rows of the array), and the NEXT brick's samples are requested before the present brick is classified,
//      so the memory latency of one brick hides behind the work on the one before.  A brick whose samples are all 1.0f or NaN
//      leaves after one barrier.  Otherwise every lane classifies its cell from LDS and the workgroup writes the brick's count.
//   2. mesh_brick_scan_kernel: one workgroup, four bricks per lane: exclusive 64-bit prefix of the counts (base of every brick) and,
//      in the same sweep, the ascending list of the bricks that have triangles.
//   3. mesh_bricks_kernel<WRITE>: the same staging over the listed bricks only; lanes interpolate and write at base + offset.
#include <new>

#include "itm_internal.h"
#include "mc_device.h"
#include "mesh_types.h"
#include "wave_utils.h"

namespace itm {

constexpr int kBrickSamples = 9 * 9 * 9;

struct BrickGrid {
  int nbx, nby, nbz;     // bricks per axis: ceil(size / 8)
  int nBricks;
};

// voxel (qx, qy, qz) of the array as a staged sample: SDF_valueToFloat, NaN where the array has none
template <class VX>
__device__ inline float brick_sample(const VolumeView& vol, uint32_t qx, uint32_t qy, uint32_t qz) {
  if (!((qx < (uint32_t)vol.sx) & (qy < (uint32_t)vol.sy) & (qz < (uint32_t)vol.sz))) return __builtin_nanf("");
  return VX::to_float(VX::load_raw_sdf(vol.vba, (size_t)qx + (size_t)qy * (size_t)vol.sx + (size_t)qz * (size_t)vol.sx * (size_t)vol.sy));
}

template <class VX, bool WRITE>
__global__ void __launch_bounds__(512) mesh_bricks_kernel(VolumeView vol, BrickGrid grid, const int32_t* __restrict__ list, const int32_t* __restrict__ nListed,
                                                          int32_t* __restrict__ brickCount, const unsigned long long* __restrict__ brickBase,
                                                          const unsigned long long* __restrict__ generatedTotal, float* __restrict__ triangles,
                                                          uint32_t maxTriangles, float factor) {
  __shared__ float sdf[kBrickSamples];        // NaN marks "no voxel stored there"
  __shared__ int scan[9];
  const int t = threadIdx.x;
  const int n = WRITE ? *nListed : grid.nBricks;
  const bool second = t + 512 < kBrickSamples;
  // sample i = x + 9 y + 81 z of the staged cube: this lane's two samples, fixed for every brick
  const int i1 = second ? t + 512 : t;
  const uint32_t x0 = t % 9, y0 = (t / 9) % 9, z0 = t / 81, x1 = i1 % 9, y1 = (i1 / 9) % 9, z1 = i1 / 81;
  const int nbxy = grid.nbx * grid.nby;
  int j = blockIdx.x;
  float r0 = 0.0f, r1 = 0.0f;
  int b = 0, bx = 0, by = 0, bz = 0;          // the brick whose samples are in r0 / r1 (uniform)
  auto request = [&]() {
    b = WRITE ? list[j] : j;
    bz = b / nbxy; by = (b - bz * nbxy) / grid.nbx; bx = b - bz * nbxy - by * grid.nbx;
    const uint32_t ox = (uint32_t)(bx * kBlockSide), oy = (uint32_t)(by * kBlockSide), oz = (uint32_t)(bz * kBlockSide);
    r0 = brick_sample<VX>(vol, ox + x0, oy + y0, oz + z0);
    if (second) r1 = brick_sample<VX>(vol, ox + x1, oy + y1, oz + z1);
  };
  if (j < n) request();
  while (j < n) {
    __syncthreads();                          // the previous brick's LDS contents are no longer needed
    sdf[t] = r0;
    if (second) sdf[t + 512] = r1;
    const bool live = (!(r0 != r0) && !(r0 == 1.0f)) || (second && !(r1 != r1) && !(r1 == 1.0f));
    const int cur = b, cbx = bx, cby = by, cbz = bz;
    // the next brick's samples are on their way while this one is classified
    j += gridDim.x;
    if (j < n) request();
    if (!__syncthreads_or(live ? 1 : 0)) {    // (uniform) every sample is 1.0f or absent: no cell of this brick survives
      if (!WRITE && t == 0) brickCount[cur] = 0;
      continue;
    }
    const int x = t & 7, y = (t >> 3) & 7, z = t >> 6;       // z outer, x inner == ascending t
    const McCell cell = classify_cell(sdf, x, y, z);
    int total;
    const int offset = block_exclusive_scan<8>(cell.nTri, scan, &total);
    if (!WRITE) {
      if (t == 0) brickCount[cur] = total;
      continue;
    }
    if (cell.nTri == 0) continue;
    // L = (array index) + denseOffset, the integer sum converted (as blockLocation + offset of the hash mesher)
    emit_cell(cell, cbx * kBlockSide + x + vol.ox, cby * kBlockSide + y + vol.oy, cbz * kBlockSide + z + vol.oz, brickBase[cur] + (unsigned long long)offset,
              *generatedTotal, maxTriangles, factor, triangles);
  }
}

// One workgroup, four bricks per lane.  brickBase[b] = triangles generated before brick b (64 bits: 2560 per brick at most, and an
// array may hold more than 2^20 bricks); list = the bricks with triangles, ascending; counters[0] = their number;
// generatedTotal = the sum; totals as mesh_scan_kernel leaves them.
__global__ void __launch_bounds__(1024) mesh_brick_scan_kernel(const int32_t* __restrict__ brickCount, int nBricks, unsigned long long* __restrict__ brickBase,
                                                               int32_t* __restrict__ list, int32_t* __restrict__ counters,
                                                               unsigned long long* __restrict__ generatedTotal, uint32_t* __restrict__ totals, uint32_t maxTriangles) {
  __shared__ int lds[17];
  __shared__ unsigned long long carry;
  __shared__ int carryListed;
  if (threadIdx.x == 0) { carry = 0ull; carryListed = 0; }
  __syncthreads();
  for (int base = 0; base < nBricks; base += 4096) {
    const int i0 = base + 4 * (int)threadIdx.x;
    int c[4], sum = 0, nonEmpty = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[k] = (i0 + k < nBricks) ? brickCount[i0 + k] : 0;
      sum += c[k];
      nonEmpty += c[k] > 0 ? 1 : 0;
    }
    int total, totalListed;
    const int ex = block_exclusive_scan<16>(sum, lds, &total);           // (both scans on one array: each begins with a barrier)
    const int exListed = block_exclusive_scan<16>(nonEmpty, lds, &totalListed);
    unsigned long long at = carry + (unsigned long long)ex;
    int slot = carryListed + exListed;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i0 + k < nBricks) {
        brickBase[i0 + k] = at;
        if (c[k] > 0) list[slot++] = i0 + k;      // slot < nBricks: at most one entry per brick
      }
      at += (unsigned long long)c[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) { carry += (unsigned long long)total; carryListed += totalListed; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counters[0] = carryListed;
    *generatedTotal = carry;
    store_triangle_totals(totals, carry, maxTriangles);
  }
}

// the dense part of itm_mesh_volume: the buffer and totals are already cleared on `st`
int launch_mesh_volume_dense(const itm_scene* s, itm_mesh* m, hipStream_t st) {
  BrickGrid g;
  g.nbx = (s->cfg.denseSize[0] + kBlockSide - 1) / kBlockSide;
  g.nby = (s->cfg.denseSize[1] + kBlockSide - 1) / kBlockSide;
  g.nbz = (s->cfg.denseSize[2] + kBlockSide - 1) / kBlockSide;
  const long long nb = (long long)g.nbx * g.nby * g.nbz;
  if (nb <= 0 || nb > 0x7fffffffll - 4096) return set_error(ITM_ERR_INVALID, "dense volume has no bricks or too many to mesh");
  g.nBricks = (int)nb;
  if (!m->brickCount) {                                         // the per-brick buffers belong to the mesh: allocated on the first dense call
    hipError_t e = m->brickCount.alloc((size_t)g.nBricks);
    if (e == hipSuccess) e = m->brickBase.alloc((size_t)g.nBricks);
    if (e == hipSuccess) e = m->brickList.alloc((size_t)g.nBricks);
    if (e == hipSuccess) e = m->brickCounters.alloc(4);     // [0] listed bricks (int32), [2..3] triangles generated (u64)
    if (e != hipSuccess) {
      m->brickCount.reset(); m->brickBase.reset(); m->brickList.reset(); m->brickCounters.reset();
      return hip_fail(e, "mesh brick buffers", __FILE__, __LINE__);
    }
  }
  const VolumeView vol = make_volume(s);
  unsigned long long* generated = (unsigned long long*)(m->brickCounters + 2);
  // persistent grid: four 512-lane workgroups fill a compute unit (2 048 lanes), 256 compute units on the MI355X -- the grid of the hash
  // mesher.  The emit pass keeps it although it strides over the listed bricks only: workgroups without a brick leave at once.
  const int launch = g.nBricks < 256 * 4 ? g.nBricks : 256 * 4;
  const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
    using VX = decltype(vx);
    mesh_bricks_kernel<VX, false><<<launch, 512, 0, st>>>(vol, g, m->brickList, m->brickCounters, m->brickCount, m->brickBase, generated, m->triangles, m->maxTriangles,
                                                          s->prm.voxelSize);
    mesh_brick_scan_kernel<<<1, 1024, 0, st>>>(m->brickCount, g.nBricks, m->brickBase, m->brickList, m->brickCounters, generated, m->totals, m->maxTriangles);
    mesh_bricks_kernel<VX, true><<<launch, 512, 0, st>>>(vol, g, m->brickList, m->brickCounters, m->brickCount, m->brickBase, generated, m->triangles, m->maxTriangles,
                                                         s->prm.voxelSize);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // namespace itm
