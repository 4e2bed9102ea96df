// volume_device.h -- the scene as kernels read it: the view of a scene's storage, the voxel look-up on every access path (sdf mirror dense
// or paged, block directory, table walk, dense array -- the same values on each) and the reads built on it.  Whatever reads a voxel
// includes this; the ray march on top of it is raycast_device.h.
//
// Reference behaviour restated (operation order: SURVEY.md Appendix A.6-A.8):
//   pointToVoxelBlockPos / readVoxel (hash, dense)  DeviceAgnostic/ITMRepresentationAccess.h:12-20, :85-142
//   readFromSDF_float_uninterpolated / _interpolated  :144-185
#pragma once

#include "itm_internal.h"
#include "itm_types.h"
#include "accel_device.h"
#include <type_traits>

namespace itm {

struct VolumeView {
  const uint4* hash;   // hash entries (hash index only)
  const void* vba;     // voxel storage
  const uint32_t* headBits;  // occupancy bitmap of the ordered buckets (hash index only)
  uint32_t mask;       // bucketNum - 1
  int bucketNum;
  const int32_t* dirPtr;    // block directory (accel_device.h); nullptr = walk the table (hash index only)
  const void* sdfMirror;    // sdf by position (accel_device.h); nullptr = none (hash index only)
  const int32_t* pageTable; // the mirror's page table as THIS kernel reads it: the scene's (memory) or the workgroup's copy in LDS (raycast_kernel)
  AccelOrigin org;          // where the directory / mirror cubes lie
  int sx, sy, sz;      // dense size
  int ox, oy, oz;      // dense offset
  // which form of the sdf mirror the code reading through this view is compiled for: -1 = decided at run time from org.mMaxPages
  // (both forms compiled in: the free-view and helper kernels), see VolumeViewM
  static constexpr int kMirror = -1;
};
// The same view for a kernel that is compiled for ONE form of the mirror (0 none, 1 dense cube, 2 paged: accel_device.h): the ray-cast
// kernel needs every tile of the image resident at once -- 4 800 waves, five per SIMD, at most 96 vector registers -- and with both
// forms' address arithmetic alive it takes 104.  Every function below takes the view as a template parameter and folds the other form away.
template <int M> struct VolumeViewM : VolumeView {
  static constexpr int kMirror = M;
  __device__ VolumeViewM(const VolumeView& v) : VolumeView(v) {}
};
template <class VOL> __device__ inline bool mirror_is_dense(const VOL& vol) { return VOL::kMirror == 1 || (VOL::kMirror < 0 && vol.org.mMaxPages < 0); }
template <class VOL> __device__ inline bool mirror_is_paged(const VOL& vol) { return VOL::kMirror == 2 || (VOL::kMirror < 0 && vol.org.mMaxPages > 0); }

// per-ray block cache: ITMVoxelBlockHash::IndexCache (Objects/ITMVoxelBlockHash.h:27-33)
struct BlockCache {
  int bx, by, bz;
  int base;
  // the mirror page the ray was last in (accel_device.h): table index and entry -- a page is 32 voxels wide, a step at most 8, so most
  // steps find their page here and go straight to the one load that follows from the position
  uint32_t pageIdx;
  int page;
  __device__ BlockCache() : bx(0x7fffffff), by(0x7fffffff), bz(0x7fffffff), base(-1), pageIdx(0xffffffffu), page(kPageNone) {}
};

// The mirror page with table index tIdx, through the per-lane cache.  The table is read by a wave only when one of its lanes has left
// its page (uniform branch; a lane that keeps its page reads entry 0 and drops it).
__device__ inline int mirror_page_of(const VolumeView& vol, bool inCube, uint32_t tIdx, BlockCache& cache) {
  const bool need = inCube && tIdx != cache.pageIdx;
  if (__any(need)) {
    const int v = vol.pageTable[need ? tIdx : 0u];
    if (need) { cache.pageIdx = tIdx; cache.page = v; }
  }
  return cache.page;
}

__device__ inline int floor_div8(int p) { return ((p < 0) ? p - 7 : p) / 8; }
// ROUND(x) = x<0 ? x-0.5 : x+0.5 (ORUtils/MathUtils.h:21-23); after the (int) truncation this equals
// x + copysign(0.5, x) for every x (they only differ for x = -0.0: -0.5 vs +0.5, both truncate to 0).
__device__ inline float round_ref(float x) { return x + __builtin_copysignf(0.5f, x); }

// Linear voxel index of integer point (px,py,pz), or -1 when no voxel is stored there.
template <bool DENSE>
__device__ inline long long locate_voxel(const VolumeView& vol, int px, int py, int pz, BlockCache& cache) {
  if (DENSE) {
    // (unsigned: 0 <= q < size in one comparison per axis; `&`, not `&&`: three compares and two ANDs instead of a ladder of
    // exec-masked branches)
    const uint32_t qx = (uint32_t)(px - vol.ox), qy = (uint32_t)(py - vol.oy), qz = (uint32_t)(pz - vol.oz);
    const bool in = (qx < (uint32_t)vol.sx) & (qy < (uint32_t)vol.sy) & (qz < (uint32_t)vol.sz);
    return in ? (long long)(qx + qy * (uint32_t)vol.sx + qz * (uint32_t)(vol.sx * vol.sy)) : -1ll;
  } else {
    const int bx = px >> 3, by = py >> 3, bz = pz >> 3;                       // floor(p / 8): arithmetic shift
    const int lin = (px & 7) + ((py & 7) << 3) + ((pz & 7) << 6);             // (p - 8 b) per axis
    if (bx == cache.bx && by == cache.by && bz == cache.bz) return (long long)cache.base + lin;
    {
      // covered by the block directory: one load instead of the table walk (same answer: the directory holds exactly
      // the entries with ptr >= 0)
      const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
      if (vol.dirPtr && dir_covers(ux, uy, uz)) {
        const int ptr = vol.dirPtr[dir_cell(ux, uy, uz)];
        if (ptr < 0) return -1;
        cache.bx = bx; cache.by = by; cache.bz = bz; cache.base = ptr * kBlockVoxels;
        return (long long)cache.base + lin;
      }
    }
    int idx = hash_index(bx, by, bz, vol.mask);
    // the 16-byte entry is only fetched when the occupancy bit says the bucket is in use
    if (!((vol.headBits[idx >> 5] >> (idx & 31)) & 1u)) return -1;
    HashEntry e = unpack_entry(vol.hash[idx]);
    for (;;) {
      if (e.px == bx && e.py == by && e.pz == bz && e.ptr >= 0) {
        cache.bx = bx; cache.by = by; cache.bz = bz; cache.base = e.ptr * kBlockVoxels;
        return (long long)cache.base + lin;
      }
      if (e.offset < 1) break;
      e = unpack_entry(vol.hash[vol.bucketNum + e.offset - 1]);
    }
    return -1;
  }
}

// Dense volumes on the ray-march path: the same index as locate_voxel<true> in 32 bits, 0xffffffff = no voxel there (a dense scene holds
// fewer than 2^32 - 1 voxels: checked at creation, scene.hip).  The 64-bit form cost the issue-bound dense ray cast two quarter-rate 64-bit
// multiply-adds in an exec-masked branch, two 64-bit comparisons and a pair of selects per voxel read (found in the ISA, round 6); here
// the products are 24-bit multiply-adds when the slice fits (sx * sy < 2^24 and every side < 2^24, a wave-uniform test).
// (qx, qy, qz): the point relative to the volume's first voxel, as unsigned (0 <= q < size in one comparison per axis).  Returns the
// linear index, 0 for a point without a voxel (always a valid address); `in` says which.
__device__ inline uint32_t dense_lin(const VolumeView& vol, uint32_t qx, uint32_t qy, uint32_t qz, bool& in, bool use = true) {
  in = use & (qx < (uint32_t)vol.sx) & (qy < (uint32_t)vol.sy) & (qz < (uint32_t)vol.sz);
  const uint32_t sx = (uint32_t)vol.sx, sxy = (uint32_t)(vol.sx * vol.sy);
  uint32_t lin;
  if ((((uint32_t)vol.sx | (uint32_t)vol.sy | (uint32_t)vol.sz | sxy) >> 24) == 0u) {      // (uniform)
    // two full-rate 24-bit multiply-adds (written out: from __umul24 with a scalar factor the compiler makes a mask and the quarter-rate
    // v_mul_lo_u32).  A lane outside the volume may have q >= 2^24: its product is not used.
    uint32_t t;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(t) : "v"(qy), "s"(sx), "v"(qx));
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(lin) : "v"(qz), "s"(sxy), "v"(t));
  } else lin = qx + qy * sx + qz * sxy;
  uint32_t r = in ? lin : 0u;
  asm("" : "+v"(r));      // (the select stays in front of the 64-bit address arithmetic: behind it, it is two selects on a shifted pair)
  return r;
}
__device__ inline uint32_t dense_lin(const VolumeView& vol, int px, int py, int pz, bool& in) {
  return dense_lin(vol, (uint32_t)(px - vol.ox), (uint32_t)(py - vol.oy), (uint32_t)(pz - vol.oz), in);
}

// raw (unconverted) sdf of the voxel at an integer point; the default voxel when absent
template <class VX, bool DENSE, class VOL = VolumeView>
__device__ inline float read_raw_sdf(const VOL& vol, int px, int py, int pz, bool& found, BlockCache& cache) {
  if constexpr (!DENSE) {
    // sdf mirror: one load, address from the position alone (same value and same "found" as the walk below: the mirror holds
    // exactly the voxels of the allocated blocks inside its cube)
    using MC = MirrorCodec<VX::kShort>;
    if (vol.sdfMirror && mirror_is_dense(vol)) {
      // DENSE cube (accel_device.h): the load is unconditional (cell 0 for a lane outside the cube) and the general path below is skipped by
      // a UNIFORM branch when every lane was served: no exec-mask bracket around the common case (ray cast 42.1 -> 41.7 us)
      const uint32_t ux = (uint32_t)((px >> 3) - vol.org.mx), uy = (uint32_t)((py >> 3) - vol.org.my), uz = (uint32_t)((pz >> 3) - vol.org.mz);
      const int mbits = mirror_dense_bits(vol.org);
      const bool covered = mirror_dense_covers(ux, uy, uz, mbits);
      const size_t mi = ((size_t)mirror_dense_cell(ux, uy, uz, mbits) << 9) | (size_t)((px & 7) + ((py & 7) << 3) + ((pz & 7) << 6));
      const typename MC::T v = ((const typename MC::T*)vol.sdfMirror)[covered ? mi : (size_t)0];
      const bool present = covered && !MC::absent(v);
      const float value = present ? MC::raw(v) : (VX::kShort ? 32767.0f : 1.0f);
      if (__all(covered)) { found = present; return value; }
      if (covered) { found = present; return value; }
    } else if (vol.sdfMirror && mirror_is_paged(vol)) {
      // PAGED cube: the page's table entry (per-lane cache, else one read), then the one load that follows from the position
      const uint32_t vx = (uint32_t)(px - (vol.org.mx << 3)), vy = (uint32_t)(py - (vol.org.my << 3)), vz = (uint32_t)(pz - (vol.org.mz << 3));      // cube-relative voxel
      const bool inCube = mirror_covers_voxel(vx, vy, vz);
      const int page = mirror_page_of(vol, inCube, mirror_table_index_voxel(vx, vy, vz), cache);
      // the page answers: with a value, or -- no block was ever allocated in it -- with "no block" and no further load
      const bool covered = inCube && page != kPageUnmappable;
      const bool mapped = covered && page >= 0;
      typename MC::T v = MC::kAbsent;
      if (__any(mapped)) {
        const size_t mi = mapped ? mirror_element(page, mirror_in_page(vx, vy, vz)) : (size_t)0;
        const typename MC::T got = ((const typename MC::T*)vol.sdfMirror)[mi];
        if (mapped) v = got;
      }
      const bool present = mapped && !MC::absent(v);
      const float value = present ? MC::raw(v) : (VX::kShort ? 32767.0f : 1.0f);
      if (__all(covered)) { found = present; return value; }
      if (covered) { found = present; return value; }
    }
  }
  if constexpr (DENSE) {
    // the load is unconditional (voxel 0 for a position outside the volume): inside an exec-masked branch the compiler waits for it there
    const uint32_t a = dense_lin(vol, px, py, pz, found);
    const float v = VX::load_raw_sdf(vol.vba, (size_t)a);
    return found ? v : (VX::kShort ? 32767.0f : 1.0f);
  } else {
    const long long a = locate_voxel<DENSE>(vol, px, py, pz, cache);
    found = a >= 0;
    if (!found) return VX::kShort ? 32767.0f : 1.0f;
    return VX::load_raw_sdf(vol.vba, (size_t)a);
  }
}

template <class VX, bool DENSE, class VOL = VolumeView>
__device__ inline float sdf_nearest(const VOL& vol, float x, float y, float z, bool& found, BlockCache& cache) {
  return VX::to_float(read_raw_sdf<VX, DENSE>(vol, (int)round_ref(x), (int)round_ref(y), (int)round_ref(z), found, cache));
}

// Walks the excess chain starting from an already loaded head entry; block base or -1.
__device__ inline int resolve_block(const VolumeView& vol, HashEntry e, int bx, int by, int bz) {
  for (;;) {
    if (e.px == bx && e.py == by && e.pz == bz && e.ptr >= 0) return e.ptr * kBlockVoxels;
    if (e.offset < 1) return -1;
    e = unpack_entry(vol.hash[vol.bucketNum + e.offset - 1]);
  }
}

// The 2x2x2 voxel neighbourhood of floor(p): raw sdf values in the reference's read order
// 000 100 | 010 110 | 001 101 | 011 111 (default value where no block is allocated).
//
// The values of a trilinear read do not depend on the order in which blocks are looked up (the
// reference's IndexCache only short-cuts the probe), so for the hash index the lookups are
// restructured for memory-level parallelism: the up-to-8 distinct blocks the neighbourhood touches
// are probed with independent loads issued back to back, then the eight voxel loads are issued
// back to back.  The nearest voxel of p (ROUND per axis) is always one of these eight corners, so
// one fetch serves both the nearest-neighbour read and the trilinear read of a ray step.
template <class VX, bool DENSE>
struct Corners {
  float v[8];      // raw sdf per corner
  bool present[8]; // block allocated / inside the dense volume
  float cx, cy, cz;  // fractional position
  int ix, iy, iz;    // floor(p)

  // Every load below is issued unconditionally from an address that is always valid (a lane that has nothing to fetch
  // reads voxel 0 / its own cell again and drops the value): a load inside an exec-masked branch forces the compiler to
  // wait for it inside that branch, which turned the eight voxel reads of a trilinear sample into eight serial round
  // trips (round 1's "4 500 cycles per trilinear step").  Unconditional, they are in flight together.
  template <class VOL>
  __device__ inline void fetch(const VOL& vol, float x, float y, float z, BlockCache& cache) {
    const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
    cx = x - fx; cy = y - fy; cz = z - fz;
    ix = (int)fx; iy = (int)fy; iz = (int)fz;
    const float dflt = VX::kShort ? 32767.0f : 1.0f;
    size_t addr[8];
    if (DENSE) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        addr[c] = (size_t)dense_lin(vol, ix + (c & 1), iy + ((c >> 1) & 1), iz + (c >> 2), present[c]);
      }
    } else {
      {
        // sdf mirror: eight independent loads.  Taken when every lane of the wave that is here can use it (a wave with a lane
        // outside the mirrored cube takes the general path as a whole: both give the same values)
        using MC = MirrorCodec<VX::kShort>;
        if (vol.sdfMirror && mirror_is_dense(vol)) {
          // DENSE cube.  The eight addresses from ONE: with the blocks in plain x-fastest order the +1 neighbour along an axis is one voxel
          // further inside the block, or -- from the block's last voxel -- the first voxel of the next block, a fixed distance either
          // way.  (Taken when the blocks of (ix, iy, iz) and of (ix, iy, iz) + 8 per axis both lie in the cube: one block more than the
          // neighbourhood needs at the cube's upper faces, where the general path gives the same values.)  ~35 vector instructions for
          // the eight addresses instead of ~140 -- half of what a trilinear read issued.
          const uint32_t mx = (uint32_t)((ix >> 3) - vol.org.mx), my = (uint32_t)((iy >> 3) - vol.org.my), mz = (uint32_t)((iz >> 3) - vol.org.mz);
          const int mbits = mirror_dense_bits(vol.org);
          const bool all = mirror_dense_covers(mx, my, mz, mbits) && mirror_dense_covers(mx + 1u, my + 1u, mz + 1u, mbits);
          const int kx = ix & 7, ky = iy & 7, kz = iz & 7;
          const size_t base = ((size_t)mirror_dense_cell(mx, my, mz, mbits) << 9) + (size_t)(kx + (ky << 3) + (kz << 6));
          const uint32_t ox = (kx == 7) ? 512u - 7u : 1u;
          const uint32_t oy = (ky == 7) ? (512u << mbits) - 56u : 8u;
          const uint32_t oz = (kz == 7) ? (512u << (2 * mbits)) - 448u : 64u;
          if (__all(all)) {
            typename MC::T m[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) m[c] = ((const typename MC::T*)vol.sdfMirror)[base + (size_t)(((c & 1) ? ox : 0u) + ((c & 2) ? oy : 0u) + ((c & 4) ? oz : 0u))];
#pragma unroll
            for (int c = 0; c < 8; ++c) { present[c] = !MC::absent(m[c]); v[c] = present[c] ? MC::raw(m[c]) : dflt; }
            return;
          }
        } else if (vol.sdfMirror && mirror_is_paged(vol)) {
          // PAGED cube.  The eight addresses from ONE: inside a page the blocks lie x-fastest at a kilobyte each, so the +1 neighbour along an axis is one
          // voxel further inside the block or -- from the block's last voxel -- the first voxel of the next block of the page, a fixed
          // distance either way (~35 vector instructions for the eight addresses instead of ~140).  That holds while the neighbourhood
          // stays inside ONE page (127 of 128 positions per axis); a wave with a lane whose neighbourhood straddles pages looks up the page
          // of each of the eight voxels instead (eight independent table reads, then the eight values).
          const uint32_t vx = (uint32_t)(ix - (vol.org.mx << 3)), vy = (uint32_t)(iy - (vol.org.my << 3)), vz = (uint32_t)(iz - (vol.org.mz << 3));
          const bool inCube = mirror_covers_voxel(vx, vy, vz) && mirror_covers_voxel(vx + 1u, vy + 1u, vz + 1u);
          const bool onePage = ((vx & kPageVoxMask) != kPageVoxMask) && ((vy & kPageVoxMask) != kPageVoxMask) && ((vz & kPageVoxMask) != kPageVoxMask);
          const typename MC::T none = MC::kAbsent;
          if (__all(inCube && onePage)) {
            const int page = mirror_page_of(vol, inCube, mirror_table_index_voxel(vx, vy, vz), cache);
            if (__all(page != kPageUnmappable)) {
              const bool mapped = page >= 0;
              typename MC::T m[8];
#pragma unroll
              for (int c = 0; c < 8; ++c) m[c] = none;
              if (__any(mapped)) {
                const size_t base = mapped ? mirror_element(page, mirror_in_page(vx, vy, vz)) : (size_t)0;
                const uint32_t ox = ((vx & 7u) == 7u) ? 512u - 7u : 1u;
                const uint32_t oy = ((vy & 7u) == 7u) ? (512u << kPageBits) - 56u : 8u;
                const uint32_t oz = ((vz & 7u) == 7u) ? (512u << (2 * kPageBits)) - 448u : 64u;
                typename MC::T got[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) got[c] = ((const typename MC::T*)vol.sdfMirror)[mapped ? base + (size_t)(((c & 1) ? ox : 0u) + ((c & 2) ? oy : 0u) + ((c & 4) ? oz : 0u)) : (size_t)0];
#pragma unroll
                for (int c = 0; c < 8; ++c) if (mapped) m[c] = got[c];
              }
#pragma unroll
              for (int c = 0; c < 8; ++c) { present[c] = !MC::absent(m[c]); v[c] = present[c] ? MC::raw(m[c]) : dflt; }
              return;
            }
          } else if (__all(inCube)) {
            // a neighbourhood that straddles pages: the page of every corner's voxel
            int pg[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) pg[c] = vol.pageTable[mirror_table_index_voxel(vx + (uint32_t)(c & 1), vy + (uint32_t)((c >> 1) & 1), vz + (uint32_t)(c >> 2))];
            bool usable = true;
#pragma unroll
            for (int c = 0; c < 8; ++c) usable &= pg[c] != kPageUnmappable;
            if (__all(usable)) {
              typename MC::T got[8];
#pragma unroll
              for (int c = 0; c < 8; ++c)
                got[c] = ((const typename MC::T*)vol.sdfMirror)[pg[c] >= 0 ? mirror_element(pg[c], mirror_in_page(vx + (uint32_t)(c & 1), vy + (uint32_t)((c >> 1) & 1), vz + (uint32_t)(c >> 2))) : (size_t)0];
#pragma unroll
              for (int c = 0; c < 8; ++c) {
                const typename MC::T mv = pg[c] >= 0 ? got[c] : none;
                present[c] = !MC::absent(mv); v[c] = present[c] ? MC::raw(mv) : dflt;
              }
              return;
            }
          }
        }
      }
      const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3;            // floor division by 8
      const int lx = ix & 7, ly = iy & 7, lz = iz & 7;
      // bit k set: the +1 neighbour along axis k lies in the next block
      const int cross = (lx == 7 ? 1 : 0) | (ly == 7 ? 2 : 0) | (lz == 7 ? 4 : 0);
      const bool cached = (bx == cache.bx && by == cache.by && bz == cache.bz);
      int base[8];
      const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
      const bool viaDir = vol.dirPtr && dir_covers(ux, uy, uz) && dir_covers(ux + 1u, uy + 1u, uz + 1u);
      // block directory: the blocks of the 2x2x2 neighbourhood are eight 4-byte cells, mostly of one 256-byte brick.  A wave
      // whose lanes all sit inside their cached block and away from its upper faces skips the round altogether.
      if (__any(viaDir && !(cached && cross == 0))) {
        int ptr[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int t = s & cross;                                     // block of corner pattern s (s itself when it crosses)
          const uint32_t cell = viaDir ? dir_cell(ux + (uint32_t)(t & 1), uy + (uint32_t)((t >> 1) & 1), uz + (uint32_t)(t >> 2)) : 0u;
          ptr[s] = vol.dirPtr[cell];
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) base[s] = (ptr[s] < 0) ? -1 : ptr[s] * kBlockVoxels;
      } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) base[s] = cache.base;             // every lane: cached && cross == 0 (or no lane uses the directory)
      }
      if (!viaDir) {
        // outside the directory (or directory disabled): table walk; entries are fetched for the blocks actually needed, the
        // other loads re-read the first entry
        const int idx0 = hash_index(bx, by, bz, vol.mask);
        HashEntry head[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const bool need = ((s & ~cross) == 0) && !(s == 0 && cached);
          head[s] = unpack_entry(vol.hash[need ? hash_index(bx + (s & 1), by + ((s >> 1) & 1), bz + (s >> 2), vol.mask) : idx0]);
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const bool need = ((s & ~cross) == 0) && !(s == 0 && cached);
          base[s] = need ? resolve_block(vol, head[s], bx + (s & 1), by + ((s >> 1) & 1), bz + (s >> 2)) : -1;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) base[s] = base[s & cross];
      }
      if (cached) {
#pragma unroll
        for (int s = 0; s < 8; ++s) if ((s & cross) == 0) base[s] = cache.base;
      } else if (base[0] >= 0) { cache.bx = bx; cache.by = by; cache.bz = bz; cache.base = base[0]; }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int b = base[c];
        const int off = ((lx + (c & 1)) & 7) + ((ly + ((c >> 1) & 1)) & 7) * 8 + ((lz + (c >> 2)) & 7) * 64;
        present[c] = b >= 0;
        addr[c] = present[c] ? (size_t)(b + off) : (size_t)0;
      }
    }
    float raw[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) raw[c] = VX::load_raw_sdf(vol.vba, addr[c]);
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = present[c] ? raw[c] : dflt;
  }

  // readFromSDF_float_interpolated on the fetched values (blend on raw values, then convert)
  __device__ inline float trilinear() const {
    float r1, r2;
    r1 = (1.0f - cx) * v[0] + cx * v[1];
    r1 = (1.0f - cy) * r1 + cy * ((1.0f - cx) * v[2] + cx * v[3]);
    r2 = (1.0f - cx) * v[4] + cx * v[5];
    r2 = (1.0f - cy) * r2 + cy * ((1.0f - cx) * v[6] + cx * v[7]);
    return VX::to_float((1.0f - cz) * r1 + cz * r2);
  }

  // readFromSDF_float_uninterpolated at the same point: the voxel at ROUND(p) is corner
  // (ROUND(p) - floor(p)) in {0,1}^3
  __device__ inline float nearest(float x, float y, float z, bool& found) const {
    // a tree of selects on the three offset bits (a chain of `if (c == k)` gets turned into a dynamically indexed
    // array by the optimiser, which then moves v[] to LDS: +30 us on the kernel)
    const bool bx = ((int)round_ref(x) - ix) != 0, by = ((int)round_ref(y) - iy) != 0, bz = ((int)round_ref(z) - iz) != 0;
    const float x0 = bx ? v[1] : v[0], x1 = bx ? v[3] : v[2], x2 = bx ? v[5] : v[4], x3 = bx ? v[7] : v[6];
    const bool p0 = bx ? present[1] : present[0], p1 = bx ? present[3] : present[2], p2 = bx ? present[5] : present[4], p3 = bx ? present[7] : present[6];
    const float y0 = by ? x1 : x0, y1 = by ? x3 : x2;
    const bool q0 = by ? p1 : p0, q1 = by ? p3 : p2;
    found = bz ? q1 : q0;
    return VX::to_float(bz ? y1 : y0);
  }
};

template <class VX, bool DENSE, class VOL = VolumeView>
__device__ inline float sdf_trilinear(const VOL& vol, float x, float y, float z, bool& found, BlockCache& cache) {
  Corners<VX, DENSE> cn;
  cn.fetch(vol, x, y, z, cache);
  found = true;
  return cn.trilinear();
}

// block base (voxel index of its first voxel) of block (bx, by, bz), or -1: directory where it covers, table walk elsewhere
__device__ inline int block_base(const VolumeView& vol, int bx, int by, int bz) {
  const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
  if (vol.dirPtr && dir_covers(ux, uy, uz)) {
    const int ptr = vol.dirPtr[dir_cell(ux, uy, uz)];
    return ptr < 0 ? -1 : ptr * kBlockVoxels;
  }
  if ((int)(int16_t)bx != bx || (int)(int16_t)by != by || (int)(int16_t)bz != bz) return -1;   // beyond the table's short coordinates
  return resolve_block(vol, unpack_entry(vol.hash[hash_index(bx, by, bz, vol.mask)]), bx, by, bz);
}

// voxel index of the first voxel of src's block (bx, by, bz), -1 where readVoxel finds none: directory where it covers, else a table
// walk that is bounded and stays inside the table (an uploaded table may hold anything); a block outside the pool counts as none
__device__ inline long long fine_block_base(const VolumeView& vol, int noTotalEntries, size_t numVoxels, int bx, int by, int bz) {
  if ((int)(int16_t)bx != bx || (int)(int16_t)by != by || (int)(int16_t)bz != bz) return -1;      // beyond the table's short coordinates
  int ptr = -1;
  const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
  if (vol.dirPtr && dir_covers(ux, uy, uz)) ptr = vol.dirPtr[dir_cell(ux, uy, uz)];
  else {
    HashEntry e = unpack_entry(vol.hash[hash_index(bx, by, bz, vol.mask)]);
    for (int steps = 0; steps <= noTotalEntries - vol.bucketNum; ++steps) {
      if (e.px == bx && e.py == by && e.pz == bz && e.ptr >= 0) { ptr = e.ptr; break; }
      if (e.offset < 1) break;
      const int next = vol.bucketNum + e.offset - 1;
      if (next >= noTotalEntries) break;
      e = unpack_entry(vol.hash[next]);
    }
  }
  if (ptr < 0 || (size_t)ptr * kBlockVoxels + kBlockVoxels > numVoxels) return -1;
  return (long long)ptr * kBlockVoxels;
}

// ---- host side: the view of a scene, and the kernel instance that reads it ------------------------------------------------------------

static inline VolumeView make_volume(const itm_scene* s) {
  VolumeView v;
  v.hash = s->hash; v.vba = s->vba; v.headBits = s->headBits;
  v.dirPtr = debug_value(ITM_DEBUG_NO_DIRECTORY) ? nullptr : s->dirPtr;
  v.sdfMirror = (debug_value(ITM_DEBUG_NO_DIRECTORY) || debug_value(ITM_DEBUG_NO_SDF_MIRROR)) ? nullptr : s->sdfMirror;
  v.pageTable = s->org.mTable;
  v.org = s->org;
  v.mask = (uint32_t)s->cfg.bucketNum - 1u; v.bucketNum = s->cfg.bucketNum;
  v.sx = s->cfg.denseSize[0]; v.sy = s->cfg.denseSize[1]; v.sz = s->cfg.denseSize[2];
  v.ox = s->cfg.denseOffset[0]; v.oy = s->cfg.denseOffset[1]; v.oz = s->cfg.denseOffset[2];
  return v;
}

// f(VX{}, std::bool_constant<DENSE>{}) for the scene's voxel type and index: the template arguments of a kernel that reads it
template <class F>
inline int dispatch_volume(const itm_scene* s, F&& f) {
  return dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
    if (s->cfg.indexType == ITM_INDEX_HASH) return f(vx, std::false_type{});
    return f(vx, std::true_type{});
  });
}

}  // namespace itm
