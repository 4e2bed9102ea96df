// merge.hip -- itm_scene_merge: fuses one TSDF scene into another on the same GPU (the "shared-map merger" the stream exchange
// gathers poses and visible lists for; include/itm_hip.h, DESIGN.md "Scene merge").
//
// Reference building blocks (no reference engine merges scenes; the operation is assembled from two that exist):
//   allocation   buildHashAllocAndVisibleTypePP's probe (DeviceAgnostic/ITMSceneReconstructionEngine.h:186-241) with block positions in
//                the place of ray steps, and the ascending sweep of DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:175-227
//   combine      CombineVoxelInformation (DeviceAgnostic/ITMSwappingEngine.h:7-69), `src` in the role of the stored block
//
// MI355X design.  A PARTICIPANT is a selected entry of `src` that holds a voxel block.  Rounds of (request, sweep): the request launch
// has one lane per src slot; a participant whose position `dst` lacks leaves its src slot + 1 in the request key of its target (an empty
// head, or the tail of the chain) with atomicMax -- the scheme of request_kernel, whose keys are (pixel, step) -- so the winner is the
// highest src slot whatever the launch order.  The sweep has one workgroup per 2048-slot chunk of dst's table; ranks in ascending slot
// order come from the per-chunk request counts the request launch left plus two scans inside the chunk (excess ranks first: an excess
// request beyond the excess list takes no voxel block, so the voxel-block ranks are scanned over the ELIGIBLE requests only).  Losers
// of a target ask again in the next round, where the winner's entry is part of the chain.  The host reads the round's counts (one
// round trip per round, as the swapping engine does per call).  Then every participant present in dst is combined by one workgroup,
// one lane per voxel: 4-, 8- or 12-byte accesses, consecutive lanes on consecutive voxels.
// Derived structures are maintained incrementally: the sweep sets the occupancy bit and the directory cells of what it allocates, the
// combine writes the block's 512 sdf values into the mirror (mapping the page if need be) -- a new block is always combined, so no
// cell is left behind; nothing is rebuilt from the table.
#include <cstring>

#include "combine_device.h"
#include "itm_internal.h"
#include "wave_utils.h"

namespace itm {

// device-side tallies of a call (ints); the host reads them after every round
enum { kMsConsidered = 0, kMsSrcWithoutBlock, kMsPresentFirst, kMsPending, kMsTargets, kMsServedBlocks, kMsServedExcess, kMsCombined, kMsDstSwappedOut,
       kMsListCount, kMsBadSlot, kMsCount = 16 };
constexpr int kWhereNot = -2, kWherePending = -1;      // per src slot: not a participant / still without a place in dst / (>= 0) its dst slot

__device__ inline void tally(int32_t* __restrict__ stats, int which, int flag) {      // one atomic per wave; every lane of the wave calls
  const int n = wave_reduce_sum(flag);
  if (n && lane_id() == 0) atomicAdd(&stats[which], n);
}

__global__ void __launch_bounds__(256) merge_mark_kernel(const int32_t* __restrict__ slots, int n, int srcEntries, uint8_t* __restrict__ sel, int32_t* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slots[i];
  if (s < 0 || s >= srcEntries) stats[kMsBadSlot] = 1;
  else sel[s] = 1;                                       // duplicates count once
}

struct MergeTable {      // dst's table as the request launch reads it
  const uint4* hash; const int32_t* dirSlot; AccelOrigin org; uint32_t mask; int bucketNum, noTotalEntries;
};

// One lane per src slot.  FIRST: who takes part (round 1); later rounds: the participants still pending.
template <bool FIRST>
__global__ void __launch_bounds__(256) merge_request_kernel(const uint4* __restrict__ srcHash, int srcEntries, const uint8_t* __restrict__ sel, int32_t* __restrict__ where,
                                                            MergeTable d, uint32_t* __restrict__ allocKey, int2* __restrict__ chunkCnt, int32_t* __restrict__ stats) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  const bool inTable = slot < srcEntries;
  HashEntry se = unpack_entry(inTable ? srcHash[slot] : make_uint4(0, 0, 0, (uint32_t)-2));
  bool pending;
  if (FIRST) {
    const bool selected = inTable && (!sel || sel[slot]);
    pending = selected && se.ptr >= 0;
    tally(stats, kMsConsidered, pending ? 1 : 0);
    tally(stats, kMsSrcWithoutBlock, (selected && se.ptr == -1) ? 1 : 0);
    if (inTable && !pending) where[slot] = kWhereNot;
  } else pending = inTable && where[slot] == kWherePending;
  int found = -1, target = -1;
  bool isExcess = false;
  if (pending) {
    const int bx = se.px, by = se.py, bz = se.pz;
    if (d.dirSlot) {          // a block that exists inside the slot directory's cube: one load
      const uint32_t ux = (uint32_t)(bx - d.org.dx), uy = (uint32_t)(by - d.org.dy), uz = (uint32_t)(bz - d.org.dz);
      if (dir_covers(ux, uy, uz)) found = d.dirSlot[dir_cell(ux, uy, uz)];
    }
    if (found < 0) {          // (also inside the cube: an entry that is swapped out has no cell)
      int idx = hash_index(bx, by, bz, d.mask);
      HashEntry he = unpack_entry(d.hash[idx]);
      if (he.px == bx && he.py == by && he.pz == bz && he.ptr >= -1) found = idx;
      else if (he.ptr >= -1) {
        isExcess = true;
        // (a chain is at most the excess region long; an uploaded table may hold anything, so the walk is bounded and stays in the table)
        for (int steps = 0; he.offset >= 1 && steps <= d.noTotalEntries - d.bucketNum; ++steps) {
          const int next = d.bucketNum + he.offset - 1;
          if (next >= d.noTotalEntries) break;
          idx = next;
          he = unpack_entry(d.hash[idx]);
          if (he.px == bx && he.py == by && he.pz == bz && he.ptr >= -1) { found = idx; break; }
        }
      }
      if (found < 0) target = idx;
    }
    if (found >= 0) where[slot] = found;
    else {
      if (FIRST) where[slot] = kWherePending;
      const uint32_t old = atomicMax(&allocKey[target], (uint32_t)slot + 1u);
      if (old == 0u) {
        atomicAdd(&chunkCnt[target / kSweepChunk].x, 1);
        if (isExcess) atomicAdd(&chunkCnt[target / kSweepChunk].y, 1);
        atomicAdd(&stats[kMsTargets], 1);
      }
    }
  }
  if (FIRST) tally(stats, kMsPresentFirst, found >= 0 ? 1 : 0);
  tally(stats, kMsPending, target >= 0 ? 1 : 0);
}

constexpr int kMergeSlotsPerThread = kSweepChunk / 256;  // 8

// The ascending sweep of one round, one workgroup per chunk of dst's table.  Sequential definition: over the slots in ascending order,
// an ordered request (empty head) is served iff a voxel block is left, an excess request (chain tail) iff a voxel block AND an excess
// entry are left; a request that is not served consumes nothing.  Hence: the excess request of excess rank e is ELIGIBLE iff
// e < excess entries available, ordered requests always are, and an eligible request of rank r among the eligible ones is served iff
// r < voxel blocks available -- it then takes allocList[last - r] and excessList[lastExcess - e].
__global__ void __launch_bounds__(256) merge_sweep_kernel(uint32_t* __restrict__ allocKey, const int2* __restrict__ chunkCnt, uint4* __restrict__ hash, int noTotalEntries, int bucketNum,
                                                          const int32_t* __restrict__ excessList, const int32_t* __restrict__ allocList, const SceneCounters* __restrict__ counters,
                                                          AccelWriter aw,
                                                          const uint4* __restrict__ srcHash, int32_t* __restrict__ where, int32_t* __restrict__ stats) {
  __shared__ int lds[16];
  const int chunk = blockIdx.x, tid = threadIdx.x;
  if (chunkCnt[chunk].x == 0) return;          // nothing requested in this chunk (uniform per workgroup)
  const int slot0 = chunk * kSweepChunk + tid * kMergeSlotsPerThread;
  uint32_t keys[kMergeSlotsPerThread];
#pragma unroll
  for (int k = 0; k < kMergeSlotsPerThread; ++k) keys[k] = slot0 + k < noTotalEntries ? allocKey[slot0 + k] : 0u;
  const int lastFreeVBA = counters->lastFreeBlockId, lastFreeExc = counters->lastFreeExcessListId;
  const int availVBA = lastFreeVBA >= 0 ? lastFreeVBA + 1 : 0, availExc = lastFreeExc >= 0 ? lastFreeExc + 1 : 0;      // a counter below -1 counts as empty
  int b1 = 0, b2 = 0;
  for (int j = tid; j < chunk; j += 256) { const int2 c = chunkCnt[j]; b1 += c.x; b2 += c.y; }
  const int baseReq = block_reduce_sum<4>(b1, lds);
  const int baseExc = block_reduce_sum<4>(b2, lds + 8);
  uint32_t excessBits = 0;
  int nExc = 0;
#pragma unroll
  for (int k = 0; k < kMergeSlotsPerThread; ++k)
    if (keys[k] && (int)hash[slot0 + k].w >= -1) { excessBits |= 1u << k; ++nExc; }      // the target of an excess request is an occupied tail, of an ordered one an empty head
  int tot;
  int re = baseExc + block_exclusive_scan<4>(nExc, lds, &tot);
  int excRank[kMergeSlotsPerThread];
  uint32_t eligibleBits = 0;
  int nElig = 0;
#pragma unroll
  for (int k = 0; k < kMergeSlotsPerThread; ++k) {
    excRank[k] = -1;
    if (!keys[k]) continue;
    if (excessBits & (1u << k)) { excRank[k] = re++; if (excRank[k] >= availExc) continue; }
    eligibleBits |= 1u << k; ++nElig;
  }
  // eligible requests of the chunks before: their ordered ones, and as many of their excess ones as the excess list serves
  int rb = (baseReq - baseExc) + (baseExc < availExc ? baseExc : availExc) + block_exclusive_scan<4>(nElig, lds + 8, &tot);
  int servedBlocks = 0, servedExcess = 0;
#pragma unroll
  for (int k = 0; k < kMergeSlotsPerThread; ++k) {
    if (!keys[k]) continue;
    const int slot = slot0 + k;
    allocKey[slot] = 0u;
    if (!(eligibleBits & (1u << k))) continue;
    const int rank = rb++;
    if (rank >= availVBA) continue;
    const int srcSlot = (int)(keys[k] - 1u);
    const HashEntry se = unpack_entry(srcHash[srcSlot]);
    const int ptr = allocList[lastFreeVBA - rank];
    int newSlot = slot;
    const bool isHead = !(excessBits & (1u << k));
    if (!isHead) {
      const int off = excessList[lastFreeExc - excRank[k]];
      if (off < 0 || bucketNum + off >= noTotalEntries) continue;        // (an uploaded excess list may hold anything)
      ((uint32_t*)&hash[slot])[2] = (uint32_t)(off + 1);                 // connect the chain tail to the child
      newSlot = bucketNum + off;
      ++servedExcess;
    }
    hash[newSlot] = pack_entry(se.px, se.py, se.pz, 0, ptr);
    aw.block_listed(newSlot, isHead, se.px, se.py, se.pz, ptr);      // (the combine below stores the block's mirror values)
    where[srcSlot] = newSlot;
    ++servedBlocks;
  }
  if (servedBlocks) atomicAdd(&stats[kMsServedBlocks], servedBlocks);
  if (servedExcess) atomicAdd(&stats[kMsServedExcess], servedExcess);
}

__global__ void merge_commit_kernel(SceneCounters* __restrict__ counters, const int32_t* __restrict__ stats) {
  // (unserved requests move no counter; a counter below -1 had nothing to serve and stays as it is)
  counters->lastFreeBlockId -= stats[kMsServedBlocks];
  counters->lastFreeExcessListId -= stats[kMsServedExcess];
}

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

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace itm

using namespace itm;

extern "C" {

int itm_scene_merge(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, itm_merge_stats* stats, itm_stream stream) {
  if (!dst || !src) return set_error(ITM_ERR_INVALID, "scene merge: null scene");
  if (dst == src) return set_error(ITM_ERR_INVALID, "scene merge: dst and src are the same scene");
  if (dst->device != src->device) return set_error(ITM_ERR_INVALID, "scene merge: the scenes are on different devices");
  if (dst->cfg.voxelType != src->cfg.voxelType) return set_error(ITM_ERR_INVALID, "scene merge: the scenes differ in voxelType");
  if (dst->cfg.indexType != src->cfg.indexType) return set_error(ITM_ERR_INVALID, "scene merge: the scenes differ in indexType");
  if (memcmp(&dst->prm.voxelSize, &src->prm.voxelSize, sizeof(float)) != 0) return set_error(ITM_ERR_INVALID, "scene merge: the scenes differ in voxelSize");
  const bool hash = dst->cfg.indexType == ITM_INDEX_HASH;
  if (!hash) {
    if (memcmp(dst->cfg.denseSize, src->cfg.denseSize, sizeof dst->cfg.denseSize) != 0 || memcmp(dst->cfg.denseOffset, src->cfg.denseOffset, sizeof dst->cfg.denseOffset) != 0 ||
        dst->numVoxels != src->numVoxels)
      return set_error(ITM_ERR_INVALID, "scene merge: dense scenes differ in denseSize / denseOffset");
    if (srcSlots_dev) return set_error(ITM_ERR_INVALID, "scene merge: a slot list with dense scenes");
  } else if (srcSlots_dev && n < 0) return set_error(ITM_ERR_INVALID, "scene merge: negative slot count");
  { const int rc = enter_scene(dst, nullptr); if (rc) return rc; }
  { const int rc = enter_scene(src, nullptr); if (rc) return rc; }
  if (dst->aheadRs) return set_error(ITM_ERR_INVALID, "scene merge: dst holds the block requests of a frame issued ahead (itm_cancel_ahead first)");
  hipStream_t st = as_stream(stream);
  itm_merge_stats out{};
  if (!hash) {
    const int rc = dispatch_voxel(dst->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      merge_dense_kernel<VX><<<4096, 256, 0, st>>>(src->vba, dst->vba, dst->numVoxels, dst->prm.maxW);
      return ITM_OK;
    });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
    out.considered = out.combined = 1;
    if (stats) *stats = out;
    return ITM_OK;
  }

  // scratch of the call, kept with dst: tallies | where[srcEntries] | list[srcEntries] | chunkCnt[dst chunks] | sel[srcEntries]
  const size_t S = (size_t)src->noTotalEntries;
  const size_t oStats = 0, oWhere = align256(kMsCount * 4), oList = oWhere + align256(S * 4), oChunk = oList + align256(S * 4),
               oSel = oChunk + align256((size_t)dst->numChunks * 8), need = oSel + align256(S);
  ITM_HIP(dst->mergeScratch.reserve(need));
  uint8_t* base = (uint8_t*)dst->mergeScratch.get();
  int32_t* dStats = (int32_t*)(base + oStats); int32_t* where = (int32_t*)(base + oWhere); int32_t* list = (int32_t*)(base + oList);
  int2* chunkCnt = (int2*)(base + oChunk); uint8_t* sel = srcSlots_dev ? base + oSel : nullptr;
  int32_t h[kMsCount];
  auto read_stats = [&]() -> int {
    ITM_HIP(hipMemcpyAsync(h, dStats, sizeof h, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
    return ITM_OK;
  };
  ITM_HIP(hipMemsetAsync(dStats, 0, kMsCount * 4, st));
  if (sel) {
    ITM_HIP(hipMemsetAsync(sel, 0, S, st));
    if (n > 0) {
      merge_mark_kernel<<<(n + 255) / 256, 256, 0, st>>>(srcSlots_dev, n, src->noTotalEntries, sel, dStats);
      ITM_LAUNCH_CHECK();
    }
    { const int rc = read_stats(); if (rc) return rc; }
    if (h[kMsBadSlot]) return set_error(ITM_ERR_INVALID, "scene merge: a slot of the list is outside src's table");      // dst is untouched
  }
  // A dst that no frame or upload has placed its cubes for: they are empty wherever they lie; the entries this call records in them
  // fix the placement (src's where the cubes are alike), which a later view moves like any other.
  if (!dst->orgPlaced) {
    if (src->orgPlaced) {
      dst->org.dx = src->org.dx; dst->org.dy = src->org.dy; dst->org.dz = src->org.dz;
      if (dst->org.mMaxPages == src->org.mMaxPages || (dst->org.mMaxPages > 0 && src->org.mMaxPages > 0)) { dst->org.mx = src->org.mx; dst->org.my = src->org.my; dst->org.mz = src->org.mz; }
    }
    dst->orgPlaced = true;
  }
  const MergeTable table{dst->hash, g_debug_no_directory ? nullptr : dst->dirSlot, dst->org, (uint32_t)(dst->cfg.bucketNum - 1), dst->cfg.bucketNum, dst->noTotalEntries};
  const int reqGrid = (src->noTotalEntries + 255) / 256;
  for (int round = 1;; ++round) {
    ITM_HIP(hipMemsetAsync(chunkCnt, 0, (size_t)dst->numChunks * 8, st));
    ITM_HIP(hipMemsetAsync(dStats + kMsPending, 0, 4 * 4, st));      // pending, targets, served blocks, served excess entries: per round
    if (round == 1) merge_request_kernel<true><<<reqGrid, 256, 0, st>>>(src->hash, src->noTotalEntries, sel, where, table, dst->allocKey, chunkCnt, dStats);
    else merge_request_kernel<false><<<reqGrid, 256, 0, st>>>(src->hash, src->noTotalEntries, sel, where, table, dst->allocKey, chunkCnt, dStats);
    ITM_LAUNCH_CHECK();
    merge_sweep_kernel<<<dst->numChunks, 256, 0, st>>>(dst->allocKey, chunkCnt, dst->hash, dst->noTotalEntries, dst->cfg.bucketNum, dst->excessList, dst->allocList, dst->counters,
                                                       accel_writer(dst), src->hash, where, dStats);
    ITM_LAUNCH_CHECK();
    merge_commit_kernel<<<1, 1, 0, st>>>(dst->counters, dStats);
    ITM_LAUNCH_CHECK();
    { const int rc = read_stats(); if (rc) return rc; }
    out.rounds = round;
    out.allocated += h[kMsServedBlocks];
    if (h[kMsTargets] == 0) break;
    if (h[kMsServedBlocks] == 0) { out.unserved = h[kMsPending]; break; }
  }
  merge_list_kernel<<<reqGrid, 256, 0, st>>>(src->hash, src->noTotalEntries, where, dst->hash, src->numVoxels, dst->numVoxels, list, dStats);
  ITM_LAUNCH_CHECK();
  { const int rc = read_stats(); if (rc) return rc; }
  out.considered = h[kMsConsidered]; out.srcWithoutBlock = h[kMsSrcWithoutBlock]; out.alreadyPresent = h[kMsPresentFirst];
  out.combined = h[kMsCombined]; out.dstSwappedOut = h[kMsDstSwappedOut];
  if (h[kMsListCount] > 0) {
    const int count = h[kMsListCount];
    const int rc = dispatch_voxel(dst->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      merge_combine_kernel<VX><<<count, 512, 0, st>>>(list, src->hash, src->vba, where, dst->hash, dst->vba, dst->prm.maxW, accel_writer(dst));
      return ITM_OK;
    });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
  }
  if (stats) *stats = out;
  return ITM_OK;
}

}  // extern "C"
