// ordered_device.h -- the two order-preserving idioms of the kernels outside the frame loop, stated once.
//
// ORDERED COMPACTION.  The flagged elements of an array are listed in ascending order by one 256-thread workgroup per chunk of
// kSweepChunk = 2048 elements, eight consecutive elements per lane.  A flagging pass has left one count per chunk; then
//     base = chunk_base(...)                  flagged elements in the chunks before this one
//     ordered_scatter(base, mask, ...)        position of each of the lane's flagged elements: base + workgroup scan, ascending
// Users: ordered_compact_kernel below (launch_ordered_compaction: the two-pass visible list and FindVisibleBlocks in alloc.hip, the
// mesher's slot list, the forward projection's missing pixels) and pc_write_kernel (visualise_aux.hip).
// SlotBytes is a lane's eight flag bytes where the flags are the visible types of eight hash slots; flag_chunk is the flagging pass.
//
// CARRY SCAN.  carry_scan: the exclusive prefix of an array of any length by ONE workgroup (mesh_index.hip, meshing.hip).
//
// LOWER BOUND.  lower_bound: the position of a value in an ascending array, where a block's run starts after a compaction.
//
// (The one-launch visible list and the allocation sweep -- visible_list_kernel, sweep_chunk, merge_sweep_kernel -- spell the same
// steps out between their own early loads and look-backs and do not go through this header.)
#pragma once

#include "itm_internal.h"
#include "wave_utils.h"

namespace itm {

constexpr int kOrderedLds = 5;      // one LDS array for both: chunk_base uses 4 ints (block_reduce_sum<4>), ordered_scatter 5 (block_exclusive_scan<4>)

// A lane's eight slot bytes (visible types or flags of eight consecutive hash slots): two words, moved as one uint2.
struct SlotBytes {
  uint32_t w[2] = {0u, 0u};
  __device__ static SlotBytes load(const uint8_t* p) { const uint2 raw = *(const uint2*)p; SlotBytes b; b.w[0] = raw.x; b.w[1] = raw.y; return b; }
  __device__ void store(uint8_t* p) const { *(uint2*)p = make_uint2(w[0], w[1]); }
  __device__ uint32_t get(int k) const { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }
  // byte k = v; true when that changed it
  __device__ bool set(int k, uint32_t v) {
    const uint32_t old = get(k);
    w[k >> 2] = (w[k >> 2] & ~(0xffu << ((k & 3) * 8))) | (v << ((k & 3) * 8));
    return v != old;
  }
  // bit k = byte k is not zero
  __device__ uint32_t nonzero_mask() const {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m |= (get(k) != 0u ? 1u : 0u) << k;
    return m;
  }
  __device__ int count() const { return __popc(nonzero_mask()); }
};

// The flagging pass of a chunk of hash slots: flags[slot] = keep(slot) ? 1 : 0 for the lane's eight slots (n: a multiple of 8) and
// chunkCount[chunk] = the chunk's number of flags.  One 256-thread workgroup per chunk.
template <class Keep>
__device__ inline void flag_chunk(int n, uint8_t* __restrict__ flags, int32_t* __restrict__ chunkCount, Keep&& keep) {
  __shared__ int lds[4];
  const int slot0 = blockIdx.x * kSweepChunk + threadIdx.x * 8;
  SlotBytes b;
  if (slot0 < n) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (keep(slot0 + k)) b.set(k, 1u);
    b.store(flags + slot0);
  }
  const int sum = block_reduce_sum<4>(b.count(), lds);
  if (threadIdx.x == 0) chunkCount[blockIdx.x] = sum;
}

// The sum of counts[0 .. chunk): the position of the chunk's first flagged element.  Chunk 0, whose base is 0, sums all nChunks counts
// instead and its thread 0 calls publish(grand total).
// Called by every thread of a 256-thread workgroup with a uniform `chunk`.  `lds`: kOrderedLds ints; the call begins with a barrier
// and the scan of ordered_scatter does too, so the two share the array and it may have been in use before.
template <class Publish>
__device__ inline int chunk_base(const int32_t* __restrict__ counts, int nChunks, int chunk, int* lds, Publish&& publish) {
  int b = 0;
  for (int j = threadIdx.x; j < (chunk == 0 ? nChunks : chunk); j += 256) b += counts[j];
  b = block_reduce_sum<4>(b, lds);
  if (chunk != 0) return b;
  if (threadIdx.x == 0) publish(b);
  return 0;
}

// The mask of a lane's eight flags, elements i0 .. i0 + 7 of n: hash slots carry one byte each and come in multiples of 8, pixels one
// int each and in any number.
__device__ inline uint32_t flag_mask(const uint8_t* __restrict__ flags, int i0, int n) {
  return i0 < n ? SlotBytes::load(flags + i0).nonzero_mask() : 0u;
}
__device__ inline uint32_t flag_mask(const int32_t* __restrict__ flags, int i0, int n) {
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) m |= (i0 + k < n && flags[i0 + k] != 0 ? 1u : 0u) << k;
  return m;
}

// Bit k of `mask` flags element k of this lane's eight.  Calls emit(k, position) for the flagged ones, where the positions of the
// workgroup's flagged elements are base, base + 1, ... in ascending (lane, k) order.  Same calling conditions as chunk_base; lanes
// without a flag return after the scan's barriers.
template <class Emit>
__device__ inline void ordered_scatter(int base, uint32_t mask, int* lds, Emit&& emit) {
  int tot;
  int pos = base + block_exclusive_scan<4>(__popc(mask), lds, &tot);
  if (mask == 0u) return;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (mask & (1u << k)) emit(k, pos++);
}

// Exclusive prefix of load(0 .. n) by ONE workgroup of NW waves (blockDim.x == NW * 64), NW * 64 elements per sweep: calls
// store(i, prefix) for every i < n and returns the total, in every thread.  `Carry` is the type of prefix and total (the elements
// of one sweep sum to less than 2^31).  Every thread of the workgroup calls it; load and store are called with i < n only.
// The carry from sweep to sweep is the sweep's total, which block_exclusive_scan hands to every thread: it lives in a register.
template <int NW, class Carry, class Load, class Store>
__device__ inline Carry carry_scan(int n, Load&& load, Store&& store) {
  __shared__ int lds[NW + 1];
  Carry carry = 0;
  for (int base = 0; base < n; base += NW * kWave) {
    const int i = base + (int)threadIdx.x;
    int total;
    const int ex = block_exclusive_scan<NW>(i < n ? (int)load(i) : 0, lds, &total);
    if (i < n) store(i, carry + (Carry)ex);
    carry += (Carry)total;
  }
  return carry;
}

// The lower bound of `value` in the ascending a[0 .. n), T = uint32_t or int32_t holding non-negative numbers: how many elements are
// below it.  (Block starts after a compaction: mesh_index_blocks_kernel, components_blocks_kernel.)
template <class T>
__device__ inline uint32_t lower_bound(const T* __restrict__ a, uint32_t n, uint32_t value) {
  uint32_t lo = 0u, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)a[mid] < value) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// The ordered compaction as a launch, F = uint8_t or int32_t: ids[0 .. min(total, cap)) = the indices i < n with flags[i] != 0, ascending;
// *rawTotal (may be null) = their number, *cappedTotal = min(total, cap).  chunkCount[c] = flagged elements of chunk c, c < nChunks =
// ceil(n / kSweepChunk).  Byte flags: n is a multiple of 8 and `flags` 8-byte aligned.  A chunk without flags leaves at once.
template <class F>
__global__ void __launch_bounds__(256) ordered_compact_kernel(const F* __restrict__ flags, const int32_t* __restrict__ chunkCount, int nChunks, int n,
                                                              int32_t* __restrict__ ids, int cap, int32_t* __restrict__ rawTotal,
                                                              int32_t* __restrict__ cappedTotal) {
  __shared__ int lds[kOrderedLds];
  const int chunk = blockIdx.x;
  if (chunk != 0 && chunkCount[chunk] == 0) return;
  const int base = chunk_base(chunkCount, nChunks, chunk, lds, [&](int total) { if (rawTotal) *rawTotal = total; *cappedTotal = total < cap ? total : cap; });
  const int i0 = chunk * kSweepChunk + threadIdx.x * 8;
  ordered_scatter(base, flag_mask(flags, i0, n), lds, [&](int k, int pos) { if (pos < cap) ids[pos] = i0 + k; });
}
template <class F>
int launch_ordered_compaction(const F* flags, const int32_t* chunkCount, int nChunks, int n, int32_t* ids, int cap, int32_t* rawTotal,
                              int32_t* cappedTotal, hipStream_t st) {
  ordered_compact_kernel<<<nChunks, 256, 0, st>>>(flags, chunkCount, nChunks, n, ids, cap, rawTotal, cappedTotal);
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // namespace itm
