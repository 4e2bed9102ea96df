// coarsen.hip -- itm_scene_coarsen: resamples one TSDF scene into another of twice the voxel size on the same GPU (level of detail;
// include/itm_hip.h, DESIGN.md "Level of detail").  The reference has no counterpart.
//
// The coarse voxel at q is the 3 x 3 x 3 tent (1 2 1 per axis, sum 64) over the fine voxels 2q + {-1, 0, 1}^3, each tap weighted by its
// observation weight as well: integer sums for the short sdf and the colours, a double sum in a fixed tap order for the float sdf.
//
// MI355X design.  Hash: the blocks of dst come from merge's placement (merge_device.h) with the participants' positions halved.  Every
// participant then claims its dst slot with one atomic exchange on the slot's request key (zero between calls); the first claimer
// appends the slot to a list -- the set D of the definition, built without a sort, in no particular order.  One workgroup of 512 lanes
// resamples one block of D, one lane per coarse voxel.  Coarse block B needs the fine voxels 16B - 1 .. 16B + 15 per axis: 17^3 = 4 913
// taps from the 27 fine blocks 2B - 1 .. 2B + 1.  27 lanes resolve the block pointers (directory, or a bounded table walk), all lanes
// stage the taps in LDS (a packed word of weight and sdf per tap for the short types, float bits plus a weight byte for the float ones,
// a packed word of colour and colour weight: 20 to 44 KB, three to seven workgroups per CU), then every lane reads its 27 taps from
// LDS in the defined order.  Stores are whole voxels, consecutive lanes on consecutive voxels, plus the block's 512 mirror values
// (mapping the page of a block this call allocated).  The workgroup zeroes the slot's request key again.
// Dense: one lane per dst cell in a grid-stride loop, taps straight from global memory.
#include "merge_device.h"
#include "volume_device.h"

namespace itm {

constexpr int kTapSide = 17, kTaps = kTapSide * kTapSide * kTapSide;      // the fine voxels one coarse block reads, per axis and in all

// the first 32-bit word of a voxel's register image: {i16 sdf, u8 w_depth, ..} for the short types, the float sdf's bits for the others
__device__ inline uint32_t first_word(uint32_t r) { return r; }
__device__ inline uint32_t first_word(uint2 r) { return r.x; }
__device__ inline uint32_t first_word(VoxelFRgb::Reg r) { return r.a; }

// One coarse voxel: the sums of the definition, fed tap by tap in the defined order.
template <class VX>
struct CoarseVoxel {
  int A = 0, S = 0;           // sum a_k, sum a_k * sdf_k (short sdf)
  double Sd = 0.0;            // sum (double)a_k * (double)sdf_k (float sdf)
  int Bc = 0, C[3] = {0, 0, 0};

  // c: the tap's tent coefficient; sdfWord: first_word of the voxel; w: its w_depth
  __device__ void depth(int c, uint32_t sdfWord, int w) {
    const int a = c * w;
    A += a;
    if constexpr (VX::kShort) S += a * (int)(int16_t)(sdfWord & 0xffffu);
    else Sd = Sd + (double)a * (double)__uint_as_float(sdfWord);
  }
  __device__ void colour(int c, const int clr[3], int wc) {
    const int b = c * wc;
    Bc += b;
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] += b * clr[i];
  }
  __device__ static int weight(int sum, int maxW) {      // min(maxW, 255, max(1, (sum + 32) div 64))
    int w = (sum + 32) / 64;
    w = w < 1 ? 1 : w;
    w = w < 255 ? w : 255;
    return w < maxW ? w : maxW;
  }
  __device__ typename VX::Reg voxel(int maxW) const {
    typename VX::Reg r = VX::init();
    if constexpr (VX::kColor) {
      if (Bc != 0) {
        int clr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) clr[i] = (int)((2u * (uint32_t)C[i] + (uint32_t)Bc) / (2u * (uint32_t)Bc));
        r = VX::with_color(r, clr, weight(Bc, maxW));
      }
    }
    if (A != 0) {
      const int w = weight(A, maxW);
      if constexpr (VX::kShort) {
        const uint32_t mag = (2u * (uint32_t)(S < 0 ? -S : S) + (uint32_t)A) / (2u * (uint32_t)A);
        const uint32_t low = (uint32_t)(uint16_t)(int16_t)(S < 0 ? -(int)mag : (int)mag) | ((uint32_t)(w & 0xff) << 16);
        if constexpr (VX::kColor) r.x = (r.x & 0xff000000u) | low;
        else r = low;
      } else r = VX::with_depth(r, (float)(Sd / (double)A), w);
    }
    return r;
  }
};

__device__ inline int tent(int k) { return 2 - (k < 0 ? -k : k); }

template <class VX>
__global__ void __launch_bounds__(512) coarsen_block_kernel(const int32_t* __restrict__ list, VolumeView src, int srcEntries, size_t srcVoxels, const uint4* __restrict__ dstHash,
                                                            void* __restrict__ dstVba, size_t dstVoxels, int maxW, uint32_t* __restrict__ allocKey, AccelWriter aw) {
  __shared__ long long bases[27];
  __shared__ uint32_t depthTap[kTaps];                                     // short: sdf | w_depth << 16; float: the sdf's bits
  __shared__ uint8_t weightTap[VX::kShort ? 4 : (kTaps + 3) & ~3];         // float: w_depth
  __shared__ uint32_t colourTap[VX::kColor ? kTaps : 1];                   // clr[0] | clr[1] << 8 | clr[2] << 16 | w_color << 24
  const int dstSlot = list[blockIdx.x], t = threadIdx.x;
  if (t == 0) allocKey[dstSlot] = 0u;
  const HashEntry de = unpack_entry(dstHash[dstSlot]);
  if (de.ptr < 0 || (size_t)de.ptr * kBlockVoxels + kBlockVoxels > dstVoxels) return;      // swapped out of dst (uniform per workgroup)
  if (t < 27) bases[t] = fine_block_base(src, srcEntries, srcVoxels, 2 * de.px - 1 + t % 3, 2 * de.py - 1 + (t / 3) % 3, 2 * de.pz - 1 + t / 9);
  __syncthreads();
  // tap (x, y, z) of the 17^3 is fine voxel 16B - 1 + (x, y, z): block (x + 7) >> 3 of the three per axis, voxel (x + 7) & 7 inside it
  for (int i = t; i < kTaps; i += 512) {
    const int x = i % kTapSide + 7, y = (i / kTapSide) % kTapSide + 7, z = i / (kTapSide * kTapSide) + 7;
    const long long base = bases[(x >> 3) + 3 * (y >> 3) + 9 * (z >> 3)];
    typename VX::Reg r = VX::init();
    if (base >= 0) r = VX::load(src.vba, (size_t)base + (size_t)((x & 7) + ((y & 7) << 3) + ((z & 7) << 6)));
    if constexpr (VX::kShort) depthTap[i] = first_word(r) & 0x00ffffffu;
    else { depthTap[i] = first_word(r); weightTap[i] = (uint8_t)VX::w_depth(r); }
    if constexpr (VX::kColor) {
      int c[3], wc;
      VX::get_color(r, c, wc);
      colourTap[i] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)wc << 24);
    }
  }
  __syncthreads();
  // coarse voxel (lx, ly, lz) of the block: its centre tap is (2 lx + 1, 2 ly + 1, 2 lz + 1) of the 17^3
  const int centre = (2 * (t & 7) + 1) + kTapSide * ((2 * ((t >> 3) & 7) + 1) + kTapSide * (2 * (t >> 6) + 1));
  CoarseVoxel<VX> cv;
#pragma unroll
  for (int kz = -1; kz <= 1; ++kz)
#pragma unroll
    for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
      for (int kx = -1; kx <= 1; ++kx) {
        const int i = centre + kx + kTapSide * (ky + kTapSide * kz), c = tent(kx) * tent(ky) * tent(kz);
        const uint32_t d = depthTap[i];
        cv.depth(c, d, VX::kShort ? (int)(d >> 16) : (int)weightTap[VX::kShort ? 0 : i]);
        if constexpr (VX::kColor) {
          const uint32_t cw = colourTap[i];
          const int clr[3] = {(int)(cw & 0xffu), (int)((cw >> 8) & 0xffu), (int)((cw >> 16) & 0xffu)};
          cv.colour(c, clr, (int)(cw >> 24));
        }
      }
  const typename VX::Reg r = cv.voxel(maxW);
  VX::store(dstVba, (size_t)de.ptr * kBlockVoxels + t, r);
  // the block's place in the sdf mirror (the page of a block allocated by this call is mapped here)
  size_t mbase;
  if (aw.block_base_workgroup<true>(de.px, de.py, de.pz, mbase)) aw.store_sdf<VX>(mbase, (uint32_t)t, VX::raw_sdf(r));
}

// dense index: cell i of dst from the 27 fine voxels around 2 (cell + dst's offset) in src's array
template <class VX>
__global__ void __launch_bounds__(256) coarsen_dense_kernel(VolumeView src, void* __restrict__ dstVba, int dsx, int dsy, int dsz, int dox, int doy, int doz, int maxW) {
  const size_t n = (size_t)dsx * (size_t)dsy * (size_t)dsz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int qx = (int)(i % (size_t)dsx) + dox, qy = (int)((i / (size_t)dsx) % (size_t)dsy) + doy, qz = (int)(i / ((size_t)dsx * (size_t)dsy)) + doz;
    CoarseVoxel<VX> cv;
#pragma unroll
    for (int kz = -1; kz <= 1; ++kz)
#pragma unroll
      for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
        for (int kx = -1; kx <= 1; ++kx) {
          // (64-bit: 2q may leave the int range of a scene placed far out; such a tap lies outside src's array)
          const long long px = 2ll * qx + kx - src.ox, py = 2ll * qy + ky - src.oy, pz = 2ll * qz + kz - src.oz;
          const bool in = px >= 0 && px < src.sx && py >= 0 && py < src.sy && pz >= 0 && pz < src.sz;
          typename VX::Reg r = VX::init();
          if (in) r = VX::load(src.vba, (size_t)px + (size_t)py * (size_t)src.sx + (size_t)pz * (size_t)src.sx * (size_t)src.sy);
          const int c = tent(kx) * tent(ky) * tent(kz);
          cv.depth(c, first_word(r), VX::w_depth(r));
          if constexpr (VX::kColor) {
            int clr[3], wc;
            VX::get_color(r, clr, wc);
            cv.colour(c, clr, wc);
          }
        }
    VX::store(dstVba, i, cv.voxel(maxW));
  }
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_scene_coarsen(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, itm_coarsen_stats* stats, itm_stream stream) {
  { const int rc = check_scene_pair(dst, src, "scene coarsen", true, true); if (rc) return rc; }
  { const int rc = enter_scene_pair(dst, src, srcSlots_dev, n, "scene coarsen"); if (rc) return rc; }
  const bool hash = dst->cfg.indexType == ITM_INDEX_HASH;
  hipStream_t st = as_stream(stream);
  itm_coarsen_stats out{};
  VolumeView fine = make_volume(src);
  if (!hash)
    return finish_dense(dst, out, &itm_coarsen_stats::written, stats, [&](auto vx) {
      coarsen_dense_kernel<decltype(vx)><<<4096, 256, 0, st>>>(fine, dst->vba, dst->cfg.denseSize[0], dst->cfg.denseSize[1], dst->cfg.denseSize[2], dst->cfg.denseOffset[0],
                                                               dst->cfg.denseOffset[1], dst->cfg.denseOffset[2], dst->prm.maxW);
    });

  MergePlacement pl;
  { const int rc = place_participants<1>(dst, src, srcSlots_dev, n, st, "scene coarsen", pl); if (rc) return rc; }
  out.considered = pl.h[kMsConsidered]; out.srcWithoutBlock = pl.h[kMsSrcWithoutBlock];
  return finish_placed(dst, pl, out, &itm_coarsen_stats::written, stats,
      [&] { claim_blocks_kernel<<<(src->noTotalEntries + 255) / 256, 256, 0, st>>>(src->noTotalEntries, pl.where, dst->hash, dst->numVoxels, dst->allocKey, pl.list, pl.dStats); },
      [&](auto vx, int count) {
        coarsen_block_kernel<decltype(vx)><<<count, 512, 0, st>>>(pl.list, fine, src->noTotalEntries, src->numVoxels, dst->hash, dst->vba, dst->numVoxels, dst->prm.maxW, dst->allocKey,
                                                                  accel_writer(dst));
      });
}

}  // extern "C"
