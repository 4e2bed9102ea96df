// merge_device.h -- the block placement that itm_scene_merge (merge.hip) and itm_scene_coarsen (coarsen.hip) share: which entries of
// `src` take part, and rounds of (request, ascending sweep) that give every participant's position an entry and a voxel block in `dst`
// (include/itm_hip.h, itm_scene_merge steps 1 and 2).  SHIFT is what distinguishes the two callers: a participant at block b asks for
// the position b >> SHIFT per component (arithmetic shift) -- 0: its own position (merge), 1: the block of twice the voxel size that
// holds it (coarsen), where up to eight participants share a position: one wins the target, the others find the entry next round.
// The rounds run over a POSITION SOURCE, any device array of packed entries (place_positions): merge and coarsen pass src's table
// (place_participants), itm_scene_resample (resample.hip) the list of candidate blocks it builds, packed as entries with ptr 0.
//
// Reference building blocks: buildHashAllocAndVisibleTypePP's probe (DeviceAgnostic/ITMSceneReconstructionEngine.h:186-241) with block
// positions in the place of ray steps, and the ascending sweep of DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:175-227.
//
// The request launch has one lane per src slot; a participant whose position `dst` lacks leaves its src slot + 1 in the request key of
// its target (an empty head, or the tail of the chain) with atomicMax -- the scheme of request_kernel, whose keys are (pixel, step) --
// so the winner is the highest src slot whatever the launch order.  The sweep has one workgroup per 2048-slot chunk of dst's table;
// ranks in ascending slot order come from the per-chunk request counts the request launch left plus two scans inside the chunk (excess
// ranks first: an excess request beyond the excess list takes no voxel block, so the voxel-block ranks are scanned over the ELIGIBLE
// requests only).  Losers of a target ask again in the next round, where the winner's entry is part of the chain.  The host reads the
// round's counts (one round trip per round, as the swapping engine does per call).  The sweep sets the occupancy bit and the directory
// cells of what it allocates; the caller's voxel launch stores the 512 mirror values of every block it touches.
// Host side, below the kernels: the selection by slot list, the rounds, and the tail of a call (scratch and refusals: scene_ops.h).
#pragma once

#include "itm_internal.h"
#include "scene_ops.h"
#include "wave_utils.h"

namespace itm {

// device-side tallies of a call (ints); the host reads them after every round
enum { kMsConsidered = 0, kMsSrcWithoutBlock, kMsPresentFirst, kMsPending, kMsTargets, kMsServedBlocks, kMsServedExcess, kMsCombined, kMsDstSwappedOut,
       kMsListCount, kMsBadSlot, kMsRsParticipants, kMsRsNoBlock, kMsRsOutOfRange, kMsRsCandidates /* (itm_scene_resample's own) */, kMsCount = 16 };
constexpr int kWhereNot = -2, kWherePending = -1;      // per src slot: not a participant / still without a place in dst / (>= 0) its dst slot

__device__ inline void tally(int32_t* __restrict__ stats, int which, int flag) {      // one atomic per wave; every lane of the wave calls
  const int n = wave_reduce_sum(flag);
  if (n && lane_id() == 0) atomicAdd(&stats[which], n);
}

static __global__ void __launch_bounds__(256) merge_mark_kernel(const int32_t* __restrict__ slots, int n, int srcEntries, uint8_t* __restrict__ sel, int32_t* __restrict__ stats) {
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
template <bool FIRST, int SHIFT>
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
    const int bx = se.px >> SHIFT, by = se.py >> SHIFT, bz = se.pz >> SHIFT;
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
template <int SHIFT>
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
    const int px = se.px >> SHIFT, py = se.py >> SHIFT, pz = se.pz >> SHIFT;
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
    hash[newSlot] = pack_entry(px, py, pz, 0, ptr);
    aw.block_listed(newSlot, isHead, px, py, pz, ptr);      // (the caller's voxel launch stores the block's mirror values)
    where[srcSlot] = newSlot;
    ++servedBlocks;
  }
  if (servedBlocks) atomicAdd(&stats[kMsServedBlocks], servedBlocks);
  if (servedExcess) atomicAdd(&stats[kMsServedExcess], servedExcess);
}

static __global__ void merge_commit_kernel(SceneCounters* __restrict__ counters, const int32_t* __restrict__ stats) {
  // (unserved requests move no counter; a counter below -1 had nothing to serve and stays as it is)
  counters->lastFreeBlockId -= stats[kMsServedBlocks];
  counters->lastFreeExcessListId -= stats[kMsServedExcess];
}

// The set D of itm_scene_coarsen and itm_scene_resample: one lane per entry of the position source; an entry with a place in dst claims
// that slot's request key (zero between calls), the first claimer lists the slot -- built without a sort, in no particular order.  The
// caller's voxel launch zeroes the keys again.
static __global__ void __launch_bounds__(256) claim_blocks_kernel(int srcEntries, const int32_t* __restrict__ where, const uint4* __restrict__ dstHash, size_t dstVoxels,
                                                                  uint32_t* __restrict__ allocKey, int32_t* __restrict__ list, int32_t* __restrict__ stats) {
  const int slot = blockIdx.x * blockDim.x + threadIdx.x;
  const int w = slot < srcEntries ? where[slot] : kWhereNot;
  bool first = false;
  int dp = -2;
  if (w >= 0) {
    first = atomicExch(&allocKey[w], 1u) == 0u;
    if (first) {
      dp = (int)dstHash[w].w;
      list[atomicAdd(&stats[kMsListCount], 1)] = w;      // (every claimed slot: the resampling launch zeroes its key again)
    }
  }
  // (a voxel block outside dst's pool: only an uploaded table can name one; it is left alone)
  tally(stats, kMsDstSwappedOut, (first && dp == -1) ? 1 : 0);
  tally(stats, kMsCombined, (first && dp >= 0 && (size_t)dp * kBlockVoxels + kBlockVoxels <= dstVoxels) ? 1 : 0);
}

// ---- host side: steps 1 and 2 of a call, and its tail -----------------------------------------------------------------------------------
struct MergePlacement {      // (its arrays: scene_ops.h, PlacementArena and ResampleArena)
  int32_t* dStats = nullptr; hipStream_t st = nullptr; int32_t* where = nullptr; int32_t* list = nullptr;
  int32_t h[kMsCount] = {};                         // the tallies as last read
  int rounds = 0, allocated = 0, unserved = 0;
  int read_stats() {                                // one host round trip
    ITM_HIP(hipMemcpyAsync(h, dStats, sizeof h, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
    return ITM_OK;
  }
};

// The selection by slot list.  mark_slots clears sel[0 .. srcEntries) and marks the listed slots (one outside the table raises kMsBadSlot
// in the tallies, which the caller has cleared); it reads nothing back, so a caller may queue more in front of the one round trip.
// refuse_bad_slots judges the tallies once read (ITM_ERR_INVALID, dst still untouched); select_slots: mark, read, judge.
inline int mark_slots(const int32_t* srcSlots_dev, int n, int srcEntries, uint8_t* sel, int32_t* dStats, hipStream_t st) {
  ITM_HIP(hipMemsetAsync(sel, 0, (size_t)srcEntries, st));
  if (n > 0) { merge_mark_kernel<<<(n + 255) / 256, 256, 0, st>>>(srcSlots_dev, n, srcEntries, sel, dStats); ITM_LAUNCH_CHECK(); }
  return ITM_OK;
}
inline int refuse_bad_slots(const int32_t* h, const char* what) { return h[kMsBadSlot] ? refuse(what, "a slot of the list is outside src's table") : ITM_OK; }
inline int select_slots(const int32_t* srcSlots_dev, int n, int srcEntries, uint8_t* sel, MergePlacement& p, const char* what) {
  { const int rc = mark_slots(srcSlots_dev, n, srcEntries, sel, p.dStats, p.st); if (rc) return rc; }
  { const int rc = p.read_stats(); if (rc) return rc; }
  return refuse_bad_slots(p.h, what);
}

// The rounds of step 2 over any device array of packed entries: `posHash[0 .. posEntries)` names the positions (an entry with ptr >= 0
// takes part, `sel` -- may be null -- narrows that to the selected slots), `p.where` has one int per entry.  itm_scene_merge and
// itm_scene_coarsen pass src's table, itm_scene_resample its candidate list (resample.hip).  chunkCnt: one int2 per chunk of dst's table.
template <int SHIFT>
inline int place_positions(itm_scene* dst, const uint4* posHash, int posEntries, const uint8_t* sel, int2* chunkCnt, hipStream_t st, MergePlacement& p) {
  const MergeTable table{dst->hash, debug_value(ITM_DEBUG_NO_DIRECTORY) ? nullptr : dst->dirSlot, dst->org, (uint32_t)(dst->cfg.bucketNum - 1), dst->cfg.bucketNum, dst->noTotalEntries};
  const int reqGrid = (posEntries + 255) / 256;
  for (int round = 1;; ++round) {
    ITM_HIP(hipMemsetAsync(chunkCnt, 0, (size_t)dst->numChunks * 8, st));
    static_assert(kMsTargets == kMsPending + 1 && kMsServedBlocks == kMsPending + 2 && kMsServedExcess == kMsPending + 3, "the four per-round tallies are consecutive");
    ITM_HIP(hipMemsetAsync(p.dStats + kMsPending, 0, 4 * 4, st));      // pending, targets, served blocks, served excess entries: per round
    if (round == 1) merge_request_kernel<true, SHIFT><<<reqGrid, 256, 0, st>>>(posHash, posEntries, sel, p.where, table, dst->allocKey, chunkCnt, p.dStats);
    else merge_request_kernel<false, SHIFT><<<reqGrid, 256, 0, st>>>(posHash, posEntries, sel, p.where, table, dst->allocKey, chunkCnt, p.dStats);
    ITM_LAUNCH_CHECK();
    merge_sweep_kernel<SHIFT><<<dst->numChunks, 256, 0, st>>>(dst->allocKey, chunkCnt, dst->hash, dst->noTotalEntries, dst->cfg.bucketNum, dst->excessList, dst->allocList, dst->counters,
                                                              accel_writer(dst), posHash, p.where, p.dStats);
    ITM_LAUNCH_CHECK();
    merge_commit_kernel<<<1, 1, 0, st>>>(dst->counters, p.dStats);
    ITM_LAUNCH_CHECK();
    { const int rc = p.read_stats(); if (rc) return rc; }
    p.rounds = round;
    p.allocated += p.h[kMsServedBlocks];
    if (p.h[kMsTargets] == 0) break;
    if (p.h[kMsServedBlocks] == 0) { p.unserved = p.h[kMsPending]; break; }
  }
  return ITM_OK;
}

// A dst that no frame or upload has placed its cubes for: they are empty wherever they lie; the entries a call records in them fix the
// placement (src's where the cubes are alike, around the same centre in dst's blocks), which a later view moves like any other.
// toDst(c, out): the block of dst that holds the centre c (a block of src) of one of src's cubes.
template <class ToDst>
inline void place_cubes_like(itm_scene* dst, const itm_scene* src, ToDst&& toDst) {
  if (dst->orgPlaced) return;
  if (src->orgPlaced) {
    auto centred = [&](int cx, int cy, int cz, int half, int& ox, int& oy, int& oz) {
      const int c[3] = {cx + half, cy + half, cz + half};
      int o[3];
      toDst(c, o);
      ox = o[0] - half; oy = o[1] - half; oz = o[2] - half;
    };
    centred(src->org.dx, src->org.dy, src->org.dz, kDirHalf, dst->org.dx, dst->org.dy, dst->org.dz);
    if (dst->org.mMaxPages == src->org.mMaxPages || (dst->org.mMaxPages > 0 && src->org.mMaxPages > 0)) {
      const int half = src->org.mMaxPages < 0 ? (1 << mirror_dense_bits(src->org)) / 2 : kMirrorHalf;
      centred(src->org.mx, src->org.my, src->org.mz, half, dst->org.mx, dst->org.my, dst->org.mz);
    }
  }
  dst->orgPlaced = true;
}

// Marks the selected slots (a slot outside src's table: ITM_ERR_INVALID, dst untouched), places dst's cubes if nothing has yet, and runs
// the rounds over src's table.  `what`: the entry point's name for messages.
template <int SHIFT>
inline int place_participants(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, hipStream_t st, const char* what, MergePlacement& p) {
  const PlacementArena a(kMsCount, (size_t)src->noTotalEntries, (size_t)dst->numChunks);
  ITM_HIP(dst->mergeScratch.reserve(a.L.bytes()));
  void* base = dst->mergeScratch.get();
  p.dStats = a.stats.at(base); p.where = a.where.at(base); p.list = a.list.at(base); p.st = st;
  uint8_t* sel = srcSlots_dev ? a.sel.at(base) : nullptr;
  ITM_HIP(hipMemsetAsync(p.dStats, 0, kMsCount * 4, st));
  if (sel) { const int rc = select_slots(srcSlots_dev, n, src->noTotalEntries, sel, p, what); if (rc) return rc; }
  // (c >> SHIFT is the centre of src's cube in dst's blocks; SHIFT == 0 leaves c as it is)
  place_cubes_like(dst, src, [](const int c[3], int o[3]) { for (int i = 0; i < 3; ++i) o[i] = c[i] >> SHIFT; });
  return place_positions<SHIFT>(dst, src->hash, src->noTotalEntries, sel, a.chunkCnt.at<int2>(base), st, p);
}

// The tail of a placed call.  listLaunch() fills p.list and the tallies (claim_blocks_kernel, or merge's own list); then the one round
// trip, the statistics every operation reports (done: the field that counts the blocks written) and blocks(vx, count), the caller's
// voxel launch over list[0 .. count).  *stats (may be null) is written once all has been launched.
template <class Stats, class ListLaunch, class Blocks>
inline int finish_placed(itm_scene* dst, MergePlacement& p, Stats& out, int32_t Stats::*done, Stats* stats, ListLaunch&& listLaunch, Blocks&& blocks) {
  out.rounds = p.rounds; out.allocated = p.allocated; out.unserved = p.unserved;
  listLaunch();
  ITM_LAUNCH_CHECK();
  { const int rc = p.read_stats(); if (rc) return rc; }
  out.alreadyPresent = p.h[kMsPresentFirst]; out.*done = p.h[kMsCombined]; out.dstSwappedOut = p.h[kMsDstSwappedOut];
  if (const int count = p.h[kMsListCount]; count > 0) {
    const int rc = dispatch_voxel(dst->cfg.voxelType, [&](auto vx) { blocks(vx, count); return ITM_OK; });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
  }
  if (stats) *stats = out;
  return ITM_OK;
}
// A call on dense scenes: cells(vx), the caller's grid-stride launch over dst's array; the statistics say one volume, written.
template <class Stats, class Cells>
inline int finish_dense(const itm_scene* dst, Stats& out, int32_t Stats::*done, Stats* stats, Cells&& cells) {
  const int rc = dispatch_voxel(dst->cfg.voxelType, [&](auto vx) { cells(vx); return ITM_OK; });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  out.considered = out.*done = 1;
  if (stats) *stats = out;
  return ITM_OK;
}

}  // namespace itm
