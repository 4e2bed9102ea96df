// prune.hip -- itm_scene_prune: the voxel blocks of a hash scene that carry no information go back to the pool (include/itm_hip.h,
// DESIGN.md "Scene pruning").
//
// No reference engine removes an entry; the pieces come from two that exist:
//   release      SaveToGlobalMemory's hand-back of a block to the allocation list (swapping.hip, swap_out_kernel), here with the entry
//   look-up      the table walk of readVoxel / the merge's request (DeviceAgnostic/ITMRepresentationAccess.h:85-119)
//
// MI355X design.  Six steps on one stream, nothing read back before the end:
//   classify     the part that reads the pool: every live block once.  A wave loads 64 entries (one coalesced kilobyte of the table, the
//                next group's while this group's blocks are read), then takes the blocks they hold two at a time: 16-byte loads,
//                consecutive lanes on consecutive 16 bytes (2 per lane for the 4-byte voxel, 4 for the 8-byte ones, 6 for the 12-byte
//                one), two ballots and one DPP maximum per block.  No LDS and no atomics: a wave leaves its six counts in a row of its
//                own and one small workgroup adds the rows up (thousands of waves adding to six words would queue up on them:
//                profiles/scene_merge.md).
//   candidates   one lane per entry; a first candidate walks the table for its 26 neighbours.
//   chains       one lane per bucket: buckets are independent and chains are short.
//   dropped ids  the ordered compaction of ordered_device.h over the dropped flags: rank = position on the two free lists.
//   release      one workgroup per dropped block, one lane per voxel: the initial value, "absent" in the mirror, the two directory
//                cells, the head bit, the two lists, the entry.
//   render states  per state an ordered compaction of its visible list without the dropped slots.
// Derived structures are maintained through AccelWriter, O(dropped blocks), as the swap-out does; nothing is rebuilt from the table.
#include <algorithm>
#include <cmath>

#include "itm_internal.h"
#include "ordered_device.h"
#include "scene_ops.h"
#include "wave_utils.h"

namespace itm {

// the statistics in device memory: itm_prune_stats word for word, then scratch words
enum { kPsConsidered, kPsEmpty, kPsFree, kPsWeak, kPsInBox, kPsCandidates, kPsProtected, kPsPinned, kPsDropped, kPsDroppedHeads, kPsDroppedExcess,
       kPsWithoutBlock, kPsVisibleRemoved, kPsLastFreeBlock, kPsLastFreeExcess, kPsReserved, kPsListCount, kPsRsTotal, kPsCount = 32 };
static_assert(sizeof(itm_prune_stats) == 16 * 4, "itm_prune_stats layout");

constexpr int kPartialWords = 8;      // a classifying wave's row of counts (six used)

struct PruneRule {
  int classes, protect, boxUsed, boxOnly;
  int shortThr; float floatThr; int weakMaxW;
  int bmin[3], bmax[3];
};

// (candidate before protection, forced) of an entry from its class byte alone
__device__ inline bool first_candidate(uint32_t c, const PruneRule& r, bool& forced) {
  const bool inbox = (c & ITM_PRUNE_IS_INBOX) != 0;
  forced = (r.classes & ITM_PRUNE_BOX) && inbox;
  const bool byClass = (c & (uint32_t)(r.classes & (ITM_PRUNE_EMPTY | ITM_PRUNE_FREE | ITM_PRUNE_WEAK))) != 0u && (!r.boxOnly || inbox);
  return byClass || forced;
}

// One voxel's part of the three block facts, from the word that holds its sdf and the one that holds its w_depth.
template <class VX>
__device__ inline void scan_voxel(uint32_t sdfWord, uint32_t w, const PruneRule& r, bool& observed, bool& below, uint32_t& maxW) {
  const bool obs = w > 0u;
  bool b;
  if (VX::kShort) b = (int)(int16_t)(sdfWord & 0xffffu) < r.shortThr;
  else b = !(__uint_as_float(sdfWord) >= r.floatThr);
  observed |= obs; below |= obs && b;
  maxW = w > maxW ? w : maxW;
}

// This lane's share of the 512 voxels of block `ptr`: 16-byte loads, consecutive lanes on consecutive 16 bytes.
template <class VX>
__device__ inline void scan_block(const void* __restrict__ vba, int ptr, int lane, const PruneRule& r, bool& observed, bool& below, uint32_t& maxW) {
  constexpr int kVec = kBlockVoxels * VX::kBytes / 16;      // uint4 per block: 128, 256 or 384
  const uint4* p = (const uint4*)vba + (size_t)ptr * kVec;
  if constexpr (VX::kBytes == 4) {                 // four voxels per load: {sdf | w << 16}
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint4 v = p[k * 64 + lane];
      scan_voxel<VX>(v.x, (v.x >> 16) & 0xffu, r, observed, below, maxW); scan_voxel<VX>(v.y, (v.y >> 16) & 0xffu, r, observed, below, maxW);
      scan_voxel<VX>(v.z, (v.z >> 16) & 0xffu, r, observed, below, maxW); scan_voxel<VX>(v.w, (v.w >> 16) & 0xffu, r, observed, below, maxW);
    }
  } else if constexpr (VX::kBytes == 8) {          // two voxels per load; w_depth: byte 2 of the first word (short sdf), byte 0 of the second (float)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4 v = p[k * 64 + lane];
      scan_voxel<VX>(v.x, VX::kShort ? (v.x >> 16) & 0xffu : v.y & 0xffu, r, observed, below, maxW);
      scan_voxel<VX>(v.z, VX::kShort ? (v.z >> 16) & 0xffu : v.w & 0xffu, r, observed, below, maxW);
    }
  } else {                                         // 12 bytes: four voxels are three loads, kept with one lane
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint4* q = p + (size_t)(k * 64 + lane) * 3;
      const uint4 a = q[0], b = q[1], c = q[2];
      scan_voxel<VX>(a.x, a.y & 0xffu, r, observed, below, maxW); scan_voxel<VX>(a.w, b.x & 0xffu, r, observed, below, maxW);
      scan_voxel<VX>(b.z, b.w & 0xffu, r, observed, below, maxW); scan_voxel<VX>(c.y, c.z & 0xffu, r, observed, below, maxW);
    }
  }
}

// Step 1.  dec[e] = the class bits of entry e (0: no block of the pool there).
template <class VX>
__global__ void __launch_bounds__(256) prune_classify_kernel(const uint4* __restrict__ hash, int nEntries, const void* __restrict__ vba, int nBlocks, PruneRule r,
                                                             uint8_t* __restrict__ dec, int32_t* __restrict__ partial) {
  const int lane = lane_id();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave, waves = gridDim.x * blockDim.x / kWave;
  int nHeld = 0, nWithout = 0, nEmpty = 0, nFree = 0, nWeak = 0, nInBox = 0;
  const int stride = waves * kWave;
  const uint4 none = make_uint4(0u, 0u, 0u, (uint32_t)-2);
  // the class bits of one block from its lanes' parts
  auto block_class = [&](bool observed, bool below, uint32_t maxW) {
    const bool anyObs = __ballot(observed) != 0ull, surface = __ballot(below) != 0ull;
    const uint32_t blockW = wave_reduce_umax(maxW);
    uint32_t c = !anyObs ? ITM_PRUNE_IS_EMPTY : surface ? ITM_PRUNE_IS_SURFACE : ITM_PRUNE_IS_FREE;
    if (anyObs && (int)blockW <= r.weakMaxW) c |= ITM_PRUNE_IS_WEAK;
    return c;
  };
  int base = wave * kWave;
  uint4 next = base + lane < nEntries ? hash[base + lane] : none;
  for (; base < nEntries; base += stride) {
    const int e = base + lane;
    const uint4 raw = next;
    next = base + stride + lane < nEntries ? hash[base + stride + lane] : none;      // on its way while this group's blocks are read
    const int ptr = (int)raw.w;
    const bool held = ptr >= 0 && ptr < nBlocks;
    nWithout += __popcll(__ballot(ptr >= -1 && !held));
    uint32_t mine = 0u;
    unsigned long long todo = __ballot(held);
    nHeld += __popcll(todo);
    while (todo) {            // two blocks per trip: their loads are independent (a last odd block is read twice, from cache)
      const int l0 = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int l1 = todo ? __ffsll((long long)todo) - 1 : l0;
      todo &= todo - 1ull;
      const int p0 = __shfl(ptr, l0), p1 = __shfl(ptr, l1);
      bool o0 = false, b0 = false, o1 = false, b1 = false; uint32_t w0 = 0u, w1 = 0u;
      scan_block<VX>(vba, p0, lane, r, o0, b0, w0);
      scan_block<VX>(vba, p1, lane, r, o1, b1, w1);
      const uint32_t c0 = block_class(o0, b0, w0), c1 = block_class(o1, b1, w1);
      if (lane == l0) mine = c0;
      if (lane == l1) mine = c1;
    }
    if (held && r.boxUsed) {
      const HashEntry he = unpack_entry(raw);
      if (he.px >= r.bmin[0] && he.px <= r.bmax[0] && he.py >= r.bmin[1] && he.py <= r.bmax[1] && he.pz >= r.bmin[2] && he.pz <= r.bmax[2]) mine |= ITM_PRUNE_IS_INBOX;
    }
    if (e < nEntries) dec[e] = (uint8_t)mine;
    nEmpty += __popcll(__ballot((mine & ITM_PRUNE_IS_EMPTY) != 0u)); nFree += __popcll(__ballot((mine & ITM_PRUNE_IS_FREE) != 0u));
    nWeak += __popcll(__ballot((mine & ITM_PRUNE_IS_WEAK) != 0u)); nInBox += __popcll(__ballot((mine & ITM_PRUNE_IS_INBOX) != 0u));
  }
  if (lane == 0) {
    int32_t* row = partial + (size_t)wave * kPartialWords;
    row[0] = nHeld; row[1] = nWithout; row[2] = nEmpty; row[3] = nFree; row[4] = nWeak; row[5] = nInBox;
  }
}

// the rows of the classifying waves added up into the statistics.  One workgroup.
__global__ void __launch_bounds__(1024) prune_tally_kernel(const int32_t* __restrict__ partial, int rows, int32_t* __restrict__ stats) {
  __shared__ int lds[16];
  const int word[6] = {kPsConsidered, kPsWithoutBlock, kPsEmpty, kPsFree, kPsWeak, kPsInBox};
  int sum[6] = {0, 0, 0, 0, 0, 0};
  for (int r = threadIdx.x; r < rows; r += 1024)
#pragma unroll
    for (int k = 0; k < 6; ++k) sum[k] += partial[(size_t)r * kPartialWords + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int total = block_reduce_sum<16>(sum[k], lds);
    if (threadIdx.x == 0) stats[word[k]] = total;
  }
}

// the slot of the entry at (bx, by, bz) with ptr >= -1, or -1: the walk of the merge's request
__device__ inline int prune_find(const uint4* __restrict__ hash, int bucketNum, int nEntries, int bx, int by, int bz) {
  int idx = hash_index(bx, by, bz, (uint32_t)(bucketNum - 1));
  HashEntry e = unpack_entry(hash[idx]);
  if (e.ptr >= -1 && e.px == bx && e.py == by && e.pz == bz) return idx;
  if (e.ptr < -1) return -1;
  for (int steps = 0; e.offset >= 1 && steps < nEntries; ++steps) {
    idx = bucketNum + e.offset - 1;
    if (idx < bucketNum || idx >= nEntries) return -1;      // (an uploaded table may hold anything)
    e = unpack_entry(hash[idx]);
    if (e.ptr >= -1 && e.px == bx && e.py == by && e.pz == bz) return idx;
  }
  return -1;
}

// Step 2.  The low five bits of a byte are final when this launch starts and are all it reads of another entry's byte.
__global__ void __launch_bounds__(256) prune_candidate_kernel(const uint4* __restrict__ hash, int nEntries, int bucketNum, PruneRule r, uint8_t* dec,
                                                              int32_t* __restrict__ stats) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nEntries) return;
  const uint32_t c = dec[e];
  bool forced;
  if (!first_candidate(c, r, forced)) return;
  bool keep = false;
  if (r.protect && !forced) {
    const HashEntry he = unpack_entry(hash[e]);
    for (int k = 0; k < 27 && !keep; ++k) {
      if (k == 13) continue;
      const int bx = he.px + k % 3 - 1, by = he.py + (k / 3) % 3 - 1, bz = he.pz + k / 9 - 1;
      if (bx < -32768 || bx > 32767 || by < -32768 || by > 32767 || bz < -32768 || bz > 32767) continue;
      const int s = prune_find(hash, bucketNum, nEntries, bx, by, bz);
      if (s < 0) continue;
      const uint32_t cs = dec[s];
      bool f;
      keep = (cs & ITM_PRUNE_IS_SURFACE) != 0u && !first_candidate(cs, r, f);
    }
  }
  if (keep) atomicAdd(&stats[kPsProtected], 1);
  else { dec[e] = (uint8_t)(c | ITM_PRUNE_IS_CANDIDATE); atomicAdd(&stats[kPsCandidates], 1); }
}

// Step 3.  One lane per bucket.  WRITE: the offsets of the entries that stay are rewritten (the dropped entries themselves are
// written by the release, which still needs their ptr).
template <bool WRITE>
__global__ void __launch_bounds__(256) prune_chain_kernel(uint4* hash, int nEntries, int bucketNum, uint8_t* dec, uint8_t* __restrict__ flags,
                                                          int32_t* __restrict__ chunkCount, int32_t* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= bucketNum) return;
  const HashEntry head = unpack_entry(hash[b]);
  if (head.ptr < -1) return;
  auto drop = [&](int slot) {
    dec[slot] |= ITM_PRUNE_IS_DROPPED;
    flags[slot] = 1;
    atomicAdd(&chunkCount[slot / kSweepChunk], 1);
    atomicAdd(&stats[slot < bucketNum ? kPsDroppedHeads : kPsDroppedExcess], 1);
    atomicAdd(&stats[kPsDropped], 1);
  };
  int prev = b, off = head.offset, survivors = 0;
  for (int steps = 0; off >= 1 && steps < nEntries - bucketNum; ++steps) {
    const int idx = bucketNum + off - 1;
    if (idx < bucketNum || idx >= nEntries) break;
    const int next = (int)hash[idx].z;
    if (dec[idx] & ITM_PRUNE_IS_CANDIDATE) {
      drop(idx);
      if (WRITE) ((uint32_t*)&hash[prev])[2] = (uint32_t)next;
    } else { ++survivors; prev = idx; }
    off = next;
  }
  if (dec[b] & ITM_PRUNE_IS_CANDIDATE) {
    if (survivors == 0) drop(b);
    else atomicAdd(&stats[kPsPinned], 1);
  }
}

// Step 4, the counters: as they become (the statistics), and with WRITE in the scene.  After the release, which reads the old ones.
template <bool WRITE>
__global__ void prune_commit_kernel(SceneCounters* __restrict__ counters, int localBlockNum, int excessNum, int32_t* __restrict__ stats) {
  const int L = counters->lastFreeBlockId < -1 ? -1 : counters->lastFreeBlockId, E = counters->lastFreeExcessListId < -1 ? -1 : counters->lastFreeExcessListId;
  int nl = L + stats[kPsDropped], ne = E + stats[kPsDroppedExcess];
  nl = nl < localBlockNum - 1 ? nl : localBlockNum - 1;
  ne = ne < excessNum - 1 ? ne : excessNum - 1;
  stats[kPsLastFreeBlock] = nl; stats[kPsLastFreeExcess] = ne;
  if (WRITE) { counters->lastFreeBlockId = nl; counters->lastFreeExcessListId = ne; }
}

// Step 4, the blocks.  ids[0 .. stats[kPsListCount]): the dropped slots, ascending.  One workgroup per dropped block at a time.
template <class VX>
__global__ void __launch_bounds__(512) prune_release_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ stats, uint4* hash, void* __restrict__ vba,
                                                            int32_t* __restrict__ allocList, int32_t* __restrict__ excessList, const SceneCounters* __restrict__ counters,
                                                            int bucketNum, int nEntries, int localBlockNum, int excessNum, AccelWriter aw) {
  __shared__ uint4 rawShared;
  const int t = threadIdx.x, n = stats[kPsListCount], nHeads = stats[kPsDroppedHeads];
  const int L = counters->lastFreeBlockId < -1 ? -1 : counters->lastFreeBlockId, E = counters->lastFreeExcessListId < -1 ? -1 : counters->lastFreeExcessListId;
  for (int rank = blockIdx.x; rank < n; rank += gridDim.x) {
    const int slot = ids[rank];
    __syncthreads();                       // (the last round's readers of rawShared)
    if (t == 0) rawShared = hash[slot];
    __syncthreads();
    const HashEntry he = unpack_entry(rawShared);
    if (he.ptr < 0 || he.ptr >= localBlockNum) continue;      // (uniform; cannot happen: only entries with a block of the pool are candidates)
    VX::store(vba, (size_t)he.ptr * kBlockVoxels + t, VX::init());
    size_t mbase;
    if (aw.block_base_wave_uniform<false>(he.px, he.py, he.pz, mbase)) aw.store_absent<VX>(mbase, (uint32_t)t);
    if (t == 0) {
      if (L + 1 + rank < localBlockNum) allocList[L + 1 + rank] = he.ptr;
      if (slot >= bucketNum) {
        const int er = E + 1 + (rank - nHeads);      // (ascending ids: the dropped heads come first)
        if (er >= 0 && er < excessNum) excessList[er] = slot - bucketNum;
      } else aw.head_released(slot);
      aw.block_released(he.px, he.py, he.pz);
      hash[slot] = pack_entry(0, 0, 0, 0, -2);
    }
  }
}

// Step 5, one render state.  The lane's eight list positions i0 .. i0 + 7: bit k = position i0 + k is listed and its slot stays.
__device__ inline uint32_t rs_keep_mask(const int32_t* __restrict__ ids, int nVis, const uint8_t* __restrict__ dec, int nEntries, int i0, int& listed) {
  uint32_t m = 0u;
  listed = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (i0 + k >= nVis) break;
    ++listed;
    const int slot = ids[i0 + k];
    const bool gone = slot >= 0 && slot < nEntries && (dec[slot] & ITM_PRUNE_IS_DROPPED) != 0;
    m |= (gone ? 0u : 1u) << k;
  }
  return m;
}
__global__ void __launch_bounds__(256) prune_rs_count_kernel(const int32_t* __restrict__ ids, const RenderCounters* __restrict__ rc, int capIds, const uint8_t* __restrict__ dec,
                                                             int nEntries, int32_t* __restrict__ chunkCount, int32_t* __restrict__ stats) {
  __shared__ int lds[kOrderedLds];
  const int nVis = min(max(rc->noVisibleEntries, 0), capIds);
  int listed;
  const uint32_t m = rs_keep_mask(ids, nVis, dec, nEntries, blockIdx.x * kSweepChunk + threadIdx.x * 8, listed);
  const int kept = block_reduce_sum<4>(__popc(m), lds), all = block_reduce_sum<4>(listed, lds);
  if (threadIdx.x == 0) {
    chunkCount[blockIdx.x] = kept;
    if (all - kept) atomicAdd(&stats[kPsVisibleRemoved], all - kept);
  }
}
__global__ void __launch_bounds__(256) prune_rs_scatter_kernel(const int32_t* __restrict__ ids, const RenderCounters* __restrict__ rc, int capIds, const uint8_t* __restrict__ dec,
                                                               int nEntries, const int32_t* __restrict__ chunkCount, int nChunks, int32_t* __restrict__ tmp,
                                                               int32_t* __restrict__ stats) {
  __shared__ int lds[kOrderedLds];
  const int nVis = min(max(rc->noVisibleEntries, 0), capIds);
  const int base = chunk_base(chunkCount, nChunks, blockIdx.x, lds, [&](int total) { stats[kPsRsTotal] = total; });
  const int i0 = blockIdx.x * kSweepChunk + threadIdx.x * 8;
  int listed;
  ordered_scatter(base, rs_keep_mask(ids, nVis, dec, nEntries, i0, listed), lds, [&](int k, int pos) { if (pos < capIds) tmp[pos] = ids[i0 + k]; });
}
__global__ void __launch_bounds__(256) prune_rs_commit_kernel(int32_t* __restrict__ ids, RenderCounters* __restrict__ rc, int capIds, const int32_t* __restrict__ tmp,
                                                              const int32_t* __restrict__ dropped, uint8_t* __restrict__ visT, int nEntries,
                                                              const int32_t* __restrict__ stats) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  const int total = min(stats[kPsRsTotal], capIds), nDropped = stats[kPsListCount];
  for (int i = i0; i < total; i += stride) ids[i] = tmp[i];
  for (int i = i0; i < nDropped; i += stride) { const int slot = dropped[i]; if (slot >= 0 && slot < nEntries) visT[slot] = 0; }
  if (i0 == 0) {
    const int nVis = min(max(rc->noVisibleEntries, 0), capIds);
    rc->rawVisibleCount -= nVis - total;
    rc->noVisibleEntries = total;
  }
}

constexpr int kClassifyGrid = 2048;      // workgroups of the classifying launch at most: 8 192 waves, each over every 8 192nd group of 64 entries

}  // namespace itm

using namespace itm;

extern "C" {

int itm_prune_default_config(itm_prune_config* out) {
  if (!out) return set_error(ITM_ERR_INVALID, "prune_default_config: null argument");
  *out = itm_prune_config{};
  out->classes = ITM_PRUNE_EMPTY | ITM_PRUNE_FREE;
  out->freeSdf = 1.0f;
  out->weakMaxW = 1;
  out->protect = 1;
  return ITM_OK;
}

int itm_scene_prune(itm_scene* s, const itm_prune_config* cfg, uint8_t* decisions_dev, itm_prune_stats* stats, itm_stream stream) {
  if (!s || !cfg) return set_error(ITM_ERR_INVALID, "scene prune: null scene or config");
  if (s->cfg.indexType != ITM_INDEX_HASH) return set_error(ITM_ERR_INVALID, "scene prune: a dense scene has no blocks to give back");
  if (s->cfg.useSwapping) return set_error(ITM_ERR_INVALID, "scene prune: the scene swaps (its host cache is keyed by table slot; swapping is its way of getting blocks back)");
  const int all = ITM_PRUNE_EMPTY | ITM_PRUNE_FREE | ITM_PRUNE_WEAK | ITM_PRUNE_BOX;
  if (cfg->classes == 0 || (cfg->classes & ~all)) return set_error(ITM_ERR_INVALID, "scene prune: classes selects nothing, or a bit outside ITM_PRUNE_*");
  if (!std::isfinite(cfg->freeSdf) || cfg->freeSdf < -1.0f || cfg->freeSdf > 1.0f) return set_error(ITM_ERR_INVALID, "scene prune: freeSdf is not a finite value in [-1, 1]");
  if ((cfg->classes & ITM_PRUNE_WEAK) && cfg->weakMaxW < 1) return set_error(ITM_ERR_INVALID, "scene prune: weakMaxW < 1 with ITM_PRUNE_WEAK");
  const bool boxUsed = (cfg->classes & ITM_PRUNE_BOX) || cfg->boxOnly;
  if (boxUsed)
    for (int k = 0; k < 3; ++k)
      if (cfg->boxMin[k] > cfg->boxMax[k]) return set_error(ITM_ERR_INVALID, "scene prune: the box has min > max");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  { const int rc = refuse_ahead(s, "scene prune", "the scene"); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const bool write = !cfg->dryRun;

  PruneRule r{};
  r.classes = cfg->classes; r.protect = cfg->protect ? 1 : 0; r.boxUsed = boxUsed ? 1 : 0; r.boxOnly = cfg->boxOnly ? 1 : 0;
  r.shortThr = (int)(int16_t)(cfg->freeSdf * 32767.0f); r.floatThr = cfg->freeSdf; r.weakMaxW = cfg->weakMaxW;
  for (int k = 0; k < 3; ++k) { r.bmin[k] = boxUsed ? cfg->boxMin[k] : 0; r.bmax[k] = boxUsed ? cfg->boxMax[k] : 0; }

  // scratch, kept with the scene (scene_ops.h: PruneArena)
  const std::vector<itm_render_state*> states = render_states_of(s);
  const int N = s->noTotalEntries, nChunks = s->numChunks, cap = s->cfg.localBlockNum, rsChunks = (cap + kSweepChunk - 1) / kSweepChunk;
  const size_t padded = (size_t)nChunks * kSweepChunk;
  const PruneArena a(kPsCount, padded, (size_t)nChunks, (size_t)N, (size_t)cap, (size_t)rsChunks, (size_t)kClassifyGrid * 4 * kPartialWords);
  ITM_HIP(s->pruneScratch.reserve(a.L.bytes()));
  void* base = s->pruneScratch.get();
  int32_t* dStats = a.stats.at(base); uint8_t* dec = a.dec.at(base); uint8_t* flags = a.flags.at(base); int32_t* chunkCount = a.chunkCount.at(base);
  int32_t* ids = a.ids.at(base); int32_t* tmp = a.tmp.at(base); int32_t* rsChunk = a.rsChunk.at(base); int32_t* partial = a.partial.at(base);
  ITM_HIP(hipMemsetAsync(base, 0, a.L.bytes_before(a.ids), st));      // statistics, bytes, flags and chunk counts

  const int nBlocks = s->cfg.localBlockNum;
  {
    const int waves = (N + kWave - 1) / kWave, grid = std::min((waves + 3) / 4, kClassifyGrid);
    const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      prune_classify_kernel<VX><<<grid, 256, 0, st>>>(s->hash, N, s->vba, nBlocks, r, dec, partial);
      return ITM_OK;
    });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
    prune_tally_kernel<<<1, 1024, 0, st>>>(partial, grid * 4, dStats);
    ITM_LAUNCH_CHECK();
  }
  prune_candidate_kernel<<<(N + 255) / 256, 256, 0, st>>>(s->hash, N, s->cfg.bucketNum, r, dec, dStats);
  ITM_LAUNCH_CHECK();
  if (write) prune_chain_kernel<true><<<(s->cfg.bucketNum + 255) / 256, 256, 0, st>>>(s->hash, N, s->cfg.bucketNum, dec, flags, chunkCount, dStats);
  else prune_chain_kernel<false><<<(s->cfg.bucketNum + 255) / 256, 256, 0, st>>>(s->hash, N, s->cfg.bucketNum, dec, flags, chunkCount, dStats);
  ITM_LAUNCH_CHECK();
  { const int rc = launch_ordered_compaction(flags, chunkCount, nChunks, (int)padded, ids, N, (int32_t*)nullptr, dStats + kPsListCount, st); if (rc) return rc; }
  if (write) {
    const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      prune_release_kernel<VX><<<1024, 512, 0, st>>>(ids, dStats, s->hash, s->vba, s->allocList, s->excessList, s->counters, s->cfg.bucketNum, N, nBlocks, s->cfg.excessNum,
                                                     accel_writer(s));
      return ITM_OK;
    });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
    prune_commit_kernel<true><<<1, 1, 0, st>>>(s->counters, nBlocks, s->cfg.excessNum, dStats);
    ++s->tableEpoch;
  } else prune_commit_kernel<false><<<1, 1, 0, st>>>(s->counters, nBlocks, s->cfg.excessNum, dStats);
  ITM_LAUNCH_CHECK();

  for (itm_render_state* rs : states) {
    if (!rs->hash || !rs->visibleIds || !rs->visibleType) continue;
    const int capIds = std::min(rs->capIds, cap), chunks = (capIds + kSweepChunk - 1) / kSweepChunk;
    if (chunks == 0) continue;
    prune_rs_count_kernel<<<chunks, 256, 0, st>>>(rs->visibleIds, rs->counters, capIds, dec, N, rsChunk, dStats);
    ITM_LAUNCH_CHECK();
    if (!write) continue;
    prune_rs_scatter_kernel<<<chunks, 256, 0, st>>>(rs->visibleIds, rs->counters, capIds, dec, N, rsChunk, chunks, tmp, dStats);
    ITM_LAUNCH_CHECK();
    prune_rs_commit_kernel<<<64, 256, 0, st>>>(rs->visibleIds, rs->counters, capIds, tmp, ids, rs->visibleType, N, dStats);
    ITM_LAUNCH_CHECK();
  }
  if (decisions_dev) ITM_HIP(hipMemcpyAsync(decisions_dev, dec, (size_t)N, hipMemcpyDeviceToDevice, st));
  if (stats) {
    ITM_HIP(hipMemcpyAsync(stats, dStats, sizeof *stats, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
    stats->reserved = 0;
  }
  return ITM_OK;
}

}  // extern "C"
