// merge.hip -- itm_scene_merge: fuses one TSDF scene into another on the same GPU (the "shared-map merger" the stream exchange
// gathers poses and visible lists for; include/itm_hip.h, DESIGN.md "Scene merge").
//
// Reference building blocks (no reference engine merges scenes; the operation is assembled from two that exist):
//   allocation   buildHashAllocAndVisibleTypePP's probe (DeviceAgnostic/ITMSceneReconstructionEngine.h:186-241) with block positions in
//                the place of ray steps, and the ascending sweep of DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:175-227
//   combine      CombineVoxelInformation (DeviceAgnostic/ITMSwappingEngine.h:7-69), `src` in the role of the stored block
//
// MI355X design.  A PARTICIPANT is a selected entry of `src` that holds a voxel block.  Rounds of (request, sweep) give every
// participant's position an entry and a voxel block in dst: merge_device.h, shared with itm_scene_coarsen (coarsen.hip), which asks for
// the position halved.  Then every participant present in dst is combined by one workgroup, one lane per voxel: 4-, 8- or 12-byte
// accesses, consecutive lanes on consecutive voxels.
// Derived structures are maintained incrementally: the sweep sets the occupancy bit and the directory cells of what it allocates, the
// combine writes the block's 512 sdf values into the mirror (mapping the page if need be) -- a new block is always combined, so no
// cell is left behind; nothing is rebuilt from the table.
#include <cstring>

#include "combine_device.h"
#include "merge_device.h"

namespace itm {

// the participants that have a voxel block in dst, in no particular order (the combine of one does not depend on another)
__global__ void __launch_bounds__(256) merge_list_kernel(const uint4* __restrict__ srcHash, int srcEntries, const int32_t* __restrict__ where, const uint4* __restrict__ dstHash,
                                                         size_t srcVoxels, size_t dstVoxels, int32_t* __restrict__ list, int32_t* __restrict__ stats) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  const int w = slot < srcEntries ? where[slot] : kWhereNot;
  int dp = -2, sp = -2;
  if (w >= 0) { dp = (int)dstHash[w].w; sp = (int)srcHash[slot].w; }
  // (voxel blocks outside either pool: only an uploaded table can name one; it is left alone)
  const bool ok = dp >= 0 && (size_t)dp * kBlockVoxels + kBlockVoxels <= dstVoxels && sp >= 0 && (size_t)sp * kBlockVoxels + kBlockVoxels <= srcVoxels;
  tally(stats, kMsDstSwappedOut, (w >= 0 && dp == -1) ? 1 : 0);
  tally(stats, kMsCombined, ok ? 1 : 0);
  if (ok) list[atomicAdd(&stats[kMsListCount], 1)] = slot;
}

// dst block = combine_voxel(src block, dst block): one workgroup per participant, one lane per voxel
template <class VX>
__global__ void __launch_bounds__(512) merge_combine_kernel(const int32_t* __restrict__ list, const uint4* __restrict__ srcHash, const void* __restrict__ srcVba,
                                                            const int32_t* __restrict__ where, const uint4* __restrict__ dstHash, void* __restrict__ dstVba, int maxW,
                                                            AccelWriter aw) {
  const int srcSlot = list[blockIdx.x], t = threadIdx.x;
  const int sp = (int)srcHash[srcSlot].w;
  const HashEntry de = unpack_entry(dstHash[where[srcSlot]]);
  const size_t vi = (size_t)de.ptr * kBlockVoxels + t;
  const typename VX::Reg r = combine_voxel<VX>(VX::load(srcVba, (size_t)sp * kBlockVoxels + t), VX::load(dstVba, vi), maxW);
  VX::store(dstVba, vi, r);
  // the block's place in the sdf mirror (the page of a block allocated by this call is mapped here)
  size_t mbase;
  if (aw.block_base_workgroup<true>(de.px, de.py, de.pz, mbase)) aw.store_sdf<VX>(mbase, (uint32_t)t, VX::raw_sdf(r));
}

// dense index: voxel i of dst with voxel i of src
template <class VX>
__global__ void __launch_bounds__(256) merge_dense_kernel(const void* __restrict__ srcVba, void* __restrict__ dstVba, size_t n, int maxW) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    VX::store(dstVba, i, combine_voxel<VX>(VX::load(srcVba, i), VX::load(dstVba, i), maxW));
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_scene_merge(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, itm_merge_stats* stats, itm_stream stream) {
  // (mu is not compared: the combine works on the stored fractions of mu, and tests/scene_merge_terms.py defines it so)
  { const int rc = check_scene_pair(dst, src, "scene merge", false, false); if (rc) return rc; }
  const bool hash = dst->cfg.indexType == ITM_INDEX_HASH;
  if (!hash && (memcmp(dst->cfg.denseSize, src->cfg.denseSize, sizeof dst->cfg.denseSize) != 0 || memcmp(dst->cfg.denseOffset, src->cfg.denseOffset, sizeof dst->cfg.denseOffset) != 0 ||
                dst->numVoxels != src->numVoxels))
    return set_error(ITM_ERR_INVALID, "scene merge: dense scenes differ in denseSize / denseOffset");
  { const int rc = enter_scene_pair(dst, src, srcSlots_dev, n, "scene merge"); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  itm_merge_stats out{};
  if (!hash)
    return finish_dense(dst, out, &itm_merge_stats::combined, stats, [&](auto vx) { merge_dense_kernel<decltype(vx)><<<4096, 256, 0, st>>>(src->vba, dst->vba, dst->numVoxels, dst->prm.maxW); });

  MergePlacement pl;
  { const int rc = place_participants<0>(dst, src, srcSlots_dev, n, st, "scene merge", pl); if (rc) return rc; }
  out.considered = pl.h[kMsConsidered]; out.srcWithoutBlock = pl.h[kMsSrcWithoutBlock];
  return finish_placed(dst, pl, out, &itm_merge_stats::combined, stats,
      [&] { merge_list_kernel<<<(src->noTotalEntries + 255) / 256, 256, 0, st>>>(src->hash, src->noTotalEntries, pl.where, dst->hash, src->numVoxels, dst->numVoxels, pl.list, pl.dStats); },
      [&](auto vx, int count) {
        merge_combine_kernel<decltype(vx)><<<count, 512, 0, st>>>(pl.list, src->hash, src->vba, pl.where, dst->hash, dst->vba, dst->prm.maxW, accel_writer(dst));
      });
}

}  // extern "C"
