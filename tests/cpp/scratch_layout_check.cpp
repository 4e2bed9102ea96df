// Host-only check of ScratchLayout and the four scratch arenas of the scene operations (infinitam_amd/csrc/scene_ops.h).  Own main, plain
// C++, arithmetic only -- no device code, no memory behind the offsets: built with g++ and run by tests/test_scratch_layout.py, and once
// by hand under -fsanitize=address,undefined.
//   1. a few hundred layouts of up to 12 parts, element sizes 1, 4, 8 and 16, counts from 0 to a few million: every part starts on a
//      256-byte boundary, parts follow each other in declaration order without overlap, bytes() is the rounded end of the last part, a
//      part of no elements takes no room (the layout without it has the same offsets), bytes_before(first) is 0 and bytes_before of the
//      k-th part is the rounded end of the one before.
//   2. the four arenas at the smallest table the GPU tests use (bucketNum 0x400, excessNum 0x100) and at the default table: every offset
//      equals the hand-carved chain of offsets the entry points had before the arenas, restated here as plain arithmetic.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../infinitam_amd/csrc/scene_ops.h"

using namespace itm;

static unsigned long long failures = 0;
static void expect(bool ok, const char* what, unsigned long long a, unsigned long long b) {
  if (!ok && failures++ < 20) std::fprintf(stderr, "FAIL %s: %llu %llu\n", what, a, b);
}
static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }      // align256 / prune_align of the entry points before

static uint64_t rngState = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

// takes `count` elements of `size` bytes; returns the part's offset
static size_t take_sized(ScratchLayout& L, size_t size, size_t count) {
  struct E8 { uint64_t a; };
  switch (size) {
    case 1: return L.take<uint8_t>(count).offset;
    case 4: return L.take<int32_t>(count).offset;
    case 8: return L.take<E8>(count).offset;
    default: return L.take<Bytes16>(count).offset;
  }
}

static void random_layouts() {
  const size_t sizes[4] = {1, 4, 8, 16};
  for (int trial = 0; trial < 400; ++trial) {
    const int parts = 1 + (int)(rnd() % 12);
    std::vector<size_t> size(parts), count(parts), off(parts);
    ScratchLayout L;
    size_t end = 0;      // the rounded end of the part before
    for (int k = 0; k < parts; ++k) {
      size[k] = sizes[rnd() % 4];
      const uint64_t r = rnd();
      count[k] = r % 5 == 0 ? 0 : r % 5 == 1 ? (size_t)(rnd() % 300) : r % 5 == 2 ? (size_t)(256 / size[k]) * (size_t)(rnd() % 9) : (size_t)(rnd() % 4000000);
      off[k] = take_sized(L, size[k], count[k]);
      expect(off[k] % 256 == 0, "a part off a 256-byte boundary", (unsigned long long)trial, off[k]);
      expect(off[k] == end, "a part does not start at the rounded end of the one before", (unsigned long long)trial, off[k]);
      expect(L.bytes_before(ScratchPart<uint8_t>{off[k]}) == end, "bytes_before", (unsigned long long)trial, (unsigned long long)k);
      end = off[k] + round256(count[k] * size[k]);
      expect(L.bytes() == end, "bytes() is not the rounded end of the last part", L.bytes(), end);
      if (count[k] == 0) expect(L.bytes() == off[k], "a part of no elements takes room", L.bytes(), off[k]);
    }
    // the same layout without its empty parts: no other offset moves
    ScratchLayout M;
    for (int k = 0; k < parts; ++k)
      if (count[k] != 0) expect(take_sized(M, size[k], count[k]) == off[k], "an empty part moved a later one", (unsigned long long)trial, (unsigned long long)k);
    expect(M.bytes() == L.bytes(), "an empty part changed the total", M.bytes(), L.bytes());
  }
  ScratchLayout L;
  const ScratchPart<int32_t> first = L.take<int32_t>(7);
  const ScratchPart<Bytes16> second = L.take<Bytes16>(17);
  expect(L.bytes_before(first) == 0 && L.bytes_before(second) == 256 && L.bytes() == 256 + 512, "the small known layout", L.bytes_before(second), L.bytes());
}

// The chains of the entry points before the arenas, and the arenas, for one table.  kMsCount 16, kPsCount 32, kSweepChunk 2048,
// kClassifyGrid 2048 and kPartialWords 8 are the values of merge_device.h, prune.hip and itm_internal.h.
static void arenas(size_t bucketNum, size_t excessNum, size_t localBlockNum) {
  const size_t kMsCount = 16, kPsCount = 32, kSweepChunk = 2048, kClassifyGrid = 2048, kPartialWords = 8;
  const size_t S = bucketNum + excessNum, chunks = (S + kSweepChunk - 1) / kSweepChunk;
  {      // place_participants (merge_device.h); dst's table the same size as src's, and a larger one
    for (size_t dstChunks : {chunks, 3 * chunks + 1}) {
      const size_t oStats = 0, oWhere = round256(kMsCount * 4), oList = oWhere + round256(S * 4), oChunk = oList + round256(S * 4), oSel = oChunk + round256(dstChunks * 8),
                   need = oSel + round256(S);
      const PlacementArena a(kMsCount, S, dstChunks);
      expect(a.stats.offset == oStats && a.where.offset == oWhere && a.list.offset == oList && a.chunkCnt.offset == oChunk && a.sel.offset == oSel && a.L.bytes() == need,
             "PlacementArena", a.L.bytes(), need);
    }
  }
  {      // itm_scene_resample (resample.hip), for several candidate counts N
    const size_t dstChunks = chunks, srcChunks = chunks;
    const size_t oStats = 0, oChunk = round256(kMsCount * 4), oCount = oChunk + round256(dstChunks * 8), oSel = oCount + round256(srcChunks * 4), oCnt = oSel + round256(S),
                 oWhere = oCnt + round256(S);
    ResampleArena a(kMsCount, dstChunks, srcChunks, S);
    expect(a.stats.offset == oStats && a.chunkCnt.offset == oChunk && a.chunkCount.offset == oCount && a.sel.offset == oSel && a.cnt.offset == oCnt, "ResampleArena prefix",
           a.cnt.offset, oCnt);
    for (size_t N : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)1000, 64 * S, (size_t)5, (size_t)0}) {      // (grows and shrinks again)
      const size_t need = oWhere + 2 * round256(N * 4) + round256(N * 16);
      const size_t got = a.size_tail(N);
      expect(got == need && a.where.offset == oWhere && a.list.offset == oWhere + round256(N * 4) && a.cand.offset == oWhere + 2 * round256(N * 4), "ResampleArena tail", got, need);
      expect(a.L.bytes() == oWhere, "size_tail moved the prefix", a.L.bytes(), oWhere);
    }
  }
  {      // itm_scene_band_samples (align.hip): hash with and without a slot list, and a dense volume of 3 * localBlockNum * 512 + 5 voxels
    const size_t elements[3] = {S * 512, S * 512, 3 * localBlockNum * 512 + 5}, sels[3] = {S, 0, 0};
    for (int k = 0; k < 3; ++k) {
      const size_t nChunks = (elements[k] + kSweepChunk - 1) / kSweepChunk, sel = sels[k];
      const size_t oStats = 256, oCount = oStats + round256(kMsCount * 4), oBase = oCount + round256(nChunks * 4), oSel = oBase + round256(nChunks * 4), need = oSel + round256(sel);
      const BandArena a(kMsCount, nChunks, sel);
      expect(a.total.offset == 0 && a.stats.offset == oStats && a.chunkCount.offset == oCount && a.chunkBase.offset == oBase && a.sel.offset == oSel && a.L.bytes() == need,
             "BandArena", a.L.bytes(), need);
    }
  }
  {      // itm_scene_prune (prune.hip)
    const size_t N = S, nChunks = chunks, cap = localBlockNum, rsChunks = (cap + kSweepChunk - 1) / kSweepChunk, padded = nChunks * kSweepChunk;
    const size_t oStats = 0, oDec = round256(kPsCount * 4), oFlags = oDec + round256(padded), oChunk = oFlags + round256(padded), oIds = oChunk + round256(nChunks * 4),
                 oTmp = oIds + round256(N * 4), oRsChunk = oTmp + round256(cap * 4), oPart = oRsChunk + round256(rsChunks * 4),
                 need = oPart + round256(kClassifyGrid * 4 * kPartialWords * 4);
    const PruneArena a(kPsCount, padded, nChunks, N, cap, rsChunks, kClassifyGrid * 4 * kPartialWords);
    expect(a.stats.offset == oStats && a.dec.offset == oDec && a.flags.offset == oFlags && a.chunkCount.offset == oChunk && a.ids.offset == oIds && a.tmp.offset == oTmp &&
               a.rsChunk.offset == oRsChunk && a.partial.offset == oPart && a.L.bytes() == need,
           "PruneArena", a.L.bytes(), need);
    expect(a.L.bytes_before(a.ids) == oIds, "what a prune clears at its start", a.L.bytes_before(a.ids), oIds);      // memset(base, 0, oIds) before
  }
}

int main() {
  random_layouts();
  arenas(0x400, 0x100, 0x200);            // the tiny tables of the GPU tests
  arenas(0x400, 0x100, 0x1);
  arenas(0x100000, 0x20000, 0x10000);     // ITM_DEFAULT_BUCKET_NUM / _EXCESS_NUM / _LOCAL_BLOCK_NUM
  arenas(0x100000, 0x20000, 0x40000);
  static uint8_t buf[1024];
  expect((void*)ScratchPart<int32_t>{256}.at(buf) == (void*)(buf + 256) && (void*)ScratchPart<Bytes8>{512}.at<char>(buf) == (void*)(buf + 512), "at()", 0, 0);
  if (failures) { std::fprintf(stderr, "%llu failures\n", failures); return 1; }
  std::printf("scratch layout check ok: 400 layouts, 4 arenas at 4 tables\n");
  return 0;
}
