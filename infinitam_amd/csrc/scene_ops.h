// scene_ops.h -- the host frame of a scene-level entry point (itm_scene_merge, _coarsen, _resample, _band_samples, _prune), stated once:
//   ScratchLayout and the arenas   the device scratch of a call, one declaration per array (plain C++: tests/cpp/scratch_layout_check.cpp)
//   check_scene_pair, check_slot_list, enter_scene_pair, refuse_ahead      the argument refusals, in one order and with one text each
// The selection by slot list (mark_slots, select_slots) and the tail of a placed call (finish_placed, finish_dense) rest on the kernels
// of merge_device.h and stand there.  A new scene operation starts from these, not from a copy of another entry point.
#pragma once
#include <cstddef>
#include <cstdint>

namespace itm {
// Where the arrays of one device buffer start: parts are taken in order, each on a 256-byte boundary; a part of no elements takes no
// room.  Arithmetic only -- the memory belongs to a DeviceBuffer (the scenes' mergeScratch / pruneScratch, or a buffer of the call).
template <class T> struct ScratchPart {
  size_t offset = 0;
  template <class U = T> U* at(void* base) const { return (U*)((uint8_t*)base + offset); }      // (U: the device's vector type of T's size)
};
struct ScratchLayout {
  size_t end = 0;
  template <class T> ScratchPart<T> take(size_t count) { const ScratchPart<T> part{end}; end += (count * sizeof(T) + 255) & ~(size_t)255; return part; }
  size_t bytes() const { return end; }
  template <class T> size_t bytes_before(ScratchPart<T> part) const { return part.offset; }      // all that was taken in front of `part`
};
using Bytes8 = uint64_t;                    // an int2 of the device
struct Bytes16 { uint64_t lo, hi; };        // a uint4 of the device

// The four arenas.  Members are initialised in the order they are declared in: that order is the layout.
struct PlacementArena {      // merge and coarsen, kept with dst: tallies | where[S] | list[S] | chunkCnt[dst chunks] | sel[S]; S: src's entries
  ScratchLayout L; ScratchPart<int32_t> stats, where, list; ScratchPart<Bytes8> chunkCnt; ScratchPart<uint8_t> sel;
  PlacementArena(size_t tallies, size_t S, size_t dstChunks)
      : stats(L.take<int32_t>(tallies)), where(L.take<int32_t>(S)), list(L.take<int32_t>(S)), chunkCnt(L.take<Bytes8>(dstChunks)), sel(L.take<uint8_t>(S)) {}
};
// resample, kept with dst: tallies | chunkCnt[dst chunks] | chunkCount[src chunks] | sel[S] | cnt[S], then where[N] | list[N] | C[N] once
// the count pass has given N: size_tail(N) places the three behind the prefix and returns the bytes of the whole.
struct ResampleArena {
  ScratchLayout L; ScratchPart<int32_t> stats; ScratchPart<Bytes8> chunkCnt; ScratchPart<int32_t> chunkCount; ScratchPart<uint8_t> sel, cnt;
  ScratchPart<int32_t> where, list; ScratchPart<Bytes16> cand;
  ResampleArena(size_t tallies, size_t dstChunks, size_t srcChunks, size_t S)
      : stats(L.take<int32_t>(tallies)), chunkCnt(L.take<Bytes8>(dstChunks)), chunkCount(L.take<int32_t>(srcChunks)), sel(L.take<uint8_t>(S)), cnt(L.take<uint8_t>(S)) {}
  size_t size_tail(size_t N) { ScratchLayout all = L; where = all.take<int32_t>(N); list = all.take<int32_t>(N); cand = all.take<Bytes16>(N); return all.bytes(); }
};
struct BandArena {      // band samples, a buffer of the call: total | tallies | chunkCount[chunks] | chunkBase[chunks] | sel[S]; S: 0 without a slot list
  ScratchLayout L; ScratchPart<int32_t> total, stats, chunkCount, chunkBase; ScratchPart<uint8_t> sel;
  BandArena(size_t tallies, size_t chunks, size_t S)
      : total(L.take<int32_t>(1)), stats(L.take<int32_t>(tallies)), chunkCount(L.take<int32_t>(chunks)), chunkBase(L.take<int32_t>(chunks)), sel(L.take<uint8_t>(S)) {}
};
// prune, kept with the scene: statistics | decision bytes | dropped flags | chunk counts | dropped ids | list copy | list chunk counts |
// the classifying waves' rows.  A call clears everything in front of `ids`.
struct PruneArena {
  ScratchLayout L; ScratchPart<int32_t> stats; ScratchPart<uint8_t> dec, flags; ScratchPart<int32_t> chunkCount, ids, tmp, rsChunk, partial;
  PruneArena(size_t statWords, size_t padded, size_t chunks, size_t entries, size_t blocks, size_t rsChunks, size_t partialWords)
      : stats(L.take<int32_t>(statWords)), dec(L.take<uint8_t>(padded)), flags(L.take<uint8_t>(padded)), chunkCount(L.take<int32_t>(chunks)), ids(L.take<int32_t>(entries)),
        tmp(L.take<int32_t>(blocks)), rsChunk(L.take<int32_t>(rsChunks)), partial(L.take<int32_t>(partialWords)) {}
};
}  // namespace itm

#ifdef __HIPCC__
#include <cstring>
#include <string>
#include "itm_internal.h"
namespace itm {
inline int refuse(const char* what, const std::string& why) { return set_error(ITM_ERR_INVALID, std::string(what) + ": " + why); }
// The refusals every operation on a pair of scenes shares.  twice: dst's voxelSize is 2.0f * src's, not src's (bit for bit); mu: it is compared too.
inline int check_scene_pair(const itm_scene* dst, const itm_scene* src, const char* what, bool twice, bool mu) {
  if (!dst || !src) return refuse(what, "null scene");
  if (dst == src) return refuse(what, "dst and src are the same scene");
  if (dst->device != src->device) return refuse(what, "the scenes are on different devices");
  if (dst->cfg.voxelType != src->cfg.voxelType) return refuse(what, "the scenes differ in voxelType");
  if (dst->cfg.indexType != src->cfg.indexType) return refuse(what, "the scenes differ in indexType");
  const float size = twice ? 2.0f * src->prm.voxelSize : src->prm.voxelSize;
  if (memcmp(&dst->prm.voxelSize, &size, sizeof(float)) != 0) return refuse(what, twice ? "dst's voxelSize is not twice src's" : "the scenes differ in voxelSize");
  if (mu && memcmp(&dst->prm.mu, &src->prm.mu, sizeof(float)) != 0) return refuse(what, "the scenes differ in mu");
  return ITM_OK;
}
// dense: what the message calls an index without a table ("dense scenes", "a dense scene")
inline int check_slot_list(bool hash, const int32_t* srcSlots_dev, int n, const char* what, const char* dense) {
  if (!hash) return srcSlots_dev ? refuse(what, std::string("a slot list with ") + dense) : ITM_OK;
  return srcSlots_dev && n < 0 ? refuse(what, "negative slot count") : ITM_OK;
}
// who: the scene as the message names it ("dst", "the scene")
inline int refuse_ahead(const itm_scene* s, const char* what, const char* who) {
  return s->aheadRs ? refuse(what, std::string(who) + " holds the block requests of a frame issued ahead (itm_cancel_ahead first)") : ITM_OK;
}
// After the other argument refusals of a pair: the slot list's, then the recorded frames of both scenes are launched, then dst must be free.
inline int enter_scene_pair(const itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, const char* what) {
  { const int rc = check_slot_list(dst->cfg.indexType == ITM_INDEX_HASH, srcSlots_dev, n, what, "dense scenes"); if (rc) return rc; }
  { const int rc = enter_scene(dst, nullptr); if (rc) return rc; }
  { const int rc = enter_scene(src, nullptr); if (rc) return rc; }
  return refuse_ahead(dst, what, "dst");
}
}  // namespace itm
#endif
