// resample.hip -- itm_rigid_quantise and itm_scene_resample: one TSDF scene brought into another's frame by a rigid transform and fused
// into it on the same GPU (multi-session / multi-robot maps; include/itm_hip.h, DESIGN.md "Scene merge under a rigid transform").
// The reference has no counterpart.
//
// The transform is quantised once on the host (Q30, voxel units, both directions); from there on the resampling is integer arithmetic in
// a fixed order: dst voxel q reads src at p = inv q + invT rounded to 1/64 voxel, eight trilinear taps with coefficients that sum to
// 2^18, each weighted by its observation weight as well (int64 sums for the short sdf and the colours, a double sum of exact products in
// the tap order for the float sdf).  The resampled voxel is fused into dst by the combine of itm_scene_merge (combine_device.h).
//
// MI355X design.  Hash: every participant of src names the dst blocks its dilated cube can reach (at most 4 x 4 x 4, kept only where
// the block's inverse box reaches the participant back) -- the candidate list C, built in order without a sort: a count pass over src's
// table (one workgroup per 2048-slot chunk, eight slots per lane, per-chunk sums), the host reads the total and sizes the scratch, a
// fill pass repeats the walk and writes at chunk base + workgroup scan (ordered_device.h).  C, packed as hash entries with ptr 0, is the
// position source of merge's placement (merge_device.h).  The claim kernel lists the set D of dst slots; one workgroup of 512 lanes
// resamples one block of D, one lane per dst voxel: the workgroup's inverse box gives a base src block, 27 lanes resolve the 3^3 block
// bases from there (directory, or a bounded table walk) into LDS, and each lane loads its eight taps straight from global memory
// through them (profiles/resample_notes.md).  Stores are whole voxels, consecutive lanes on consecutive voxels, plus the block's 512
// mirror values; the workgroup zeroes the slot's request key again.
// Dense: one lane per dst cell in a grid-stride loop, taps through the dense index.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "combine_device.h"
#include "merge_device.h"
#include "ordered_device.h"
#include "volume_device.h"

namespace itm {

constexpr long long kQ30RowBound = 1879048192ll;      // 1.75 * 2^30: sum |entry| of a row of inv / fwd
constexpr long long kQ30MaxT = 1ll << 48;

// the first 32-bit word of a voxel's register image: {i16 sdf, u8 w_depth, ..} for the short types, the float sdf's bits for the others
__device__ inline uint32_t rs_first_word(uint32_t r) { return r; }
__device__ inline uint32_t rs_first_word(uint2 r) { return r.x; }
__device__ inline uint32_t rs_first_word(VoxelFRgb::Reg r) { return r.a; }

// The box of m * [lo3, hi3] + T per axis, in Q30: lo = T + sum_j min(m_ij lo_j, m_ij hi_j), hi the same with max.
__host__ __device__ inline void q30_box(const int32_t* m, const int64_t* T, const long long lo3[3], const long long hi3[3], long long lo[3], long long hi[3]) {
  for (int i = 0; i < 3; ++i) {
    long long l = T[i], h = T[i];
    for (int j = 0; j < 3; ++j) {
      const long long a = (long long)m[3 * i + j] * lo3[j], b = (long long)m[3 * i + j] * hi3[j];
      l += a < b ? a : b;
      h += a < b ? b : a;
    }
    lo[i] = l; hi[i] = h;
  }
}
// the voxels a Q30 box can touch with its trilinear footprint: [(lo >> 30) - 1, (hi >> 30) + 2]
__host__ __device__ inline long long q30_first(long long lo) { return (lo >> 30) - 1; }
__host__ __device__ inline long long q30_last(long long hi) { return (hi >> 30) + 2; }

// The candidates of a participant at block (bx, by, bz), in the defined order (Bz outermost, Bx innermost, ascending): emit(Bx, By, Bz) for
// each that fits the table's short coordinates; returns how many did not.
template <class Emit>
__device__ inline int for_candidates(const itm_rigid_q& q, int bx, int by, int bz, Emit&& emit) {
  const long long b[3] = {bx, by, bz};
  const long long lo3[3] = {8 * b[0] - 1, 8 * b[1] - 1, 8 * b[2] - 1}, hi3[3] = {8 * b[0] + 8, 8 * b[1] + 8, 8 * b[2] + 8};
  long long lo[3], hi[3];
  q30_box(q.fwd, q.fwdT, lo3, hi3, lo, hi);
  long long B0[3], B1[3];
  for (int i = 0; i < 3; ++i) { B0[i] = q30_first(lo[i]) >> 3; B1[i] = q30_last(hi[i]) >> 3; }
  int outOfRange = 0;
  for (long long Bz = B0[2]; Bz <= B1[2]; ++Bz)
    for (long long By = B0[1]; By <= B1[1]; ++By)
      for (long long Bx = B0[0]; Bx <= B1[0]; ++Bx) {
        const long long c0[3] = {8 * Bx, 8 * By, 8 * Bz}, c1[3] = {8 * Bx + 7, 8 * By + 7, 8 * Bz + 7};
        long long slo[3], shi[3];
        q30_box(q.inv, q.invT, c0, c1, slo, shi);
        bool reaches = true;
        for (int i = 0; i < 3; ++i) reaches = reaches && q30_first(slo[i]) <= 8 * b[i] + 7 && q30_last(shi[i]) >= 8 * b[i];
        if (!reaches) continue;
        if (Bx < -32768 || Bx > 32767 || By < -32768 || By > 32767 || Bz < -32768 || Bz > 32767) { ++outOfRange; continue; }
        emit((int)Bx, (int)By, (int)Bz);
      }
  return outOfRange;
}

// Count pass: one workgroup per chunk of src's table, eight consecutive slots per lane.  cnt[slot] = candidates of the participant there
// (0 for every other slot), chunkCount[chunk] = their sum; the participants, the selected entries without a block, the candidates out
// of range and the total are tallied.
__global__ void __launch_bounds__(256) resample_count_kernel(const uint4* __restrict__ srcHash, int srcEntries, const uint8_t* __restrict__ sel, itm_rigid_q q,
                                                             uint8_t* __restrict__ cnt, int32_t* __restrict__ chunkCount, int32_t* __restrict__ stats) {
  __shared__ int lds[4];
  const int slot0 = blockIdx.x * kSweepChunk + threadIdx.x * 8;
  int sum = 0, participants = 0, noBlock = 0, outOfRange = 0;
  for (int k = 0; k < 8; ++k) {
    const int slot = slot0 + k;
    if (slot >= srcEntries) break;
    int c = 0;
    if (!sel || sel[slot]) {
      const HashEntry se = unpack_entry(srcHash[slot]);
      if (se.ptr >= 0) {
        ++participants;
        outOfRange += for_candidates(q, se.px, se.py, se.pz, [&](int, int, int) { ++c; });
      } else if (se.ptr == -1) ++noBlock;
    }
    cnt[slot] = (uint8_t)c;      // (at most 64)
    sum += c;
  }
  tally(stats, kMsRsParticipants, participants);
  tally(stats, kMsRsNoBlock, noBlock);
  tally(stats, kMsRsOutOfRange, outOfRange);
  const int total = block_reduce_sum<4>(sum, lds);
  if (threadIdx.x == 0) {
    chunkCount[blockIdx.x] = total;
    if (total) atomicAdd(&stats[kMsRsCandidates], total);
  }
}

// Fill pass, same shape: the candidates of slot s start at (candidates of the chunks before) + (workgroup scan of the lanes before)
// + (the lane's slots before s), so C is in ascending src slot order and in walk order within a participant.
__global__ void __launch_bounds__(256) resample_fill_kernel(const uint4* __restrict__ srcHash, int srcEntries, itm_rigid_q q, const uint8_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ chunkCount, int nChunks, int capacity, uint4* __restrict__ cand) {
  __shared__ int lds[kOrderedLds];
  const int chunk = blockIdx.x;
  if (chunkCount[chunk] == 0) return;      // (uniform per workgroup)
  const int base = chunk_base(chunkCount, nChunks, chunk, lds, [](int) {});
  const int slot0 = chunk * kSweepChunk + threadIdx.x * 8;
  int mine = 0;
  for (int k = 0; k < 8 && slot0 + k < srcEntries; ++k) mine += cnt[slot0 + k];
  int tot;
  int pos = base + block_exclusive_scan<4>(mine, lds, &tot);
  if (mine == 0) return;
  for (int k = 0; k < 8 && slot0 + k < srcEntries; ++k) {
    if (cnt[slot0 + k] == 0) continue;
    const HashEntry se = unpack_entry(srcHash[slot0 + k]);
    for_candidates(q, se.px, se.py, se.pz, [&](int Bx, int By, int Bz) {
      if (pos < capacity) cand[pos] = pack_entry(Bx, By, Bz, 0, 0);
      ++pos;
    });
  }
}

// One resampled voxel: the sums of the definition, fed tap by tap in the defined order.
template <class VX>
struct ResampledVoxel {
  long long A = 0, S = 0;      // sum a_k, sum a_k * sdf_k (short sdf)
  double Sd = 0.0;             // sum (double)a_k * (double)sdf_k (float sdf)
  long long Bc = 0, C[3] = {0, 0, 0};

  // c: the tap's trilinear coefficient (0 .. 2^18); sdfWord: rs_first_word of the voxel; w: its w_depth
  __device__ void depth(int c, uint32_t sdfWord, int w) {
    const long long a = (long long)c * w;
    A += a;
    if constexpr (VX::kShort) S += a * (long long)(int16_t)(sdfWord & 0xffffu);
    else Sd = Sd + (double)a * (double)__uint_as_float(sdfWord);
  }
  __device__ void colour(int c, const int clr[3], int wc) {
    const long long b = (long long)c * wc;
    Bc += b;
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] += b * clr[i];
  }
  __device__ static int weight(long long sum) {      // min(255, max(1, (sum + 2^17) >> 18))
    const int w = (int)((sum + (1ll << 17)) >> 18);
    return w < 1 ? 1 : (w < 255 ? w : 255);
  }
  // r of the definition: a part without observations keeps TVoxel()'s values and weight 0, which the combine passes over
  __device__ typename VX::Reg voxel() const {
    typename VX::Reg r = VX::init();
    if constexpr (VX::kColor) {
      if (Bc != 0) {
        int clr[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) clr[i] = (int)((2ull * (unsigned long long)C[i] + (unsigned long long)Bc) / (2ull * (unsigned long long)Bc));
        r = VX::with_color(r, clr, weight(Bc));
      }
    }
    if (A != 0) {
      const int w = weight(A);
      if constexpr (VX::kShort) {
        const unsigned long long mag = (2ull * (unsigned long long)(S < 0 ? -S : S) + (unsigned long long)A) / (2ull * (unsigned long long)A);
        const uint32_t low = (uint32_t)(uint16_t)(int16_t)(S < 0 ? -(int)mag : (int)mag) | ((uint32_t)(w & 0xff) << 16);
        if constexpr (VX::kColor) r.x = (r.x & 0xff000000u) | low;
        else r = low;
      } else r = VX::with_depth(r, (float)(Sd / (double)A), w);
    }
    return r;
  }
};

// src position of dst voxel (qx, qy, qz) in Q6: cell f and fraction u per axis
__device__ inline void resample_position(const itm_rigid_q& q, long long qx, long long qy, long long qz, long long f[3], int u[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const long long p = (long long)q.inv[3 * i] * qx + (long long)q.inv[3 * i + 1] * qy + (long long)q.inv[3 * i + 2] * qz + (long long)q.invT[i];
    const long long P = (p + (1ll << 23)) >> 24;
    f[i] = P >> 6;
    u[i] = (int)(P & 63);
  }
}

template <class VX>
__device__ inline void resample_tap(ResampledVoxel<VX>& rv, int c, typename VX::Reg t) {
  rv.depth(c, rs_first_word(t), VX::w_depth(t));
  if constexpr (VX::kColor) {
    int clr[3], wc;
    VX::get_color(t, clr, wc);
    rv.colour(c, clr, wc);
  }
}

// The taps of a block of D either come straight from global memory through the 27 block bases (STAGED false) or from a 16^3 footprint
// of src staged in LDS first (STAGED true): the taps of a block span at most 15 voxels per axis from lo >> 30 of its inverse box on.
// Both give the same bits; profiles/resample_notes.md has the two times on the MI355X and the choice (ITM_RESAMPLE_STAGED).
#ifndef ITM_RESAMPLE_STAGED
#define ITM_RESAMPLE_STAGED 0
#endif
constexpr int kFootSide = 16, kFoot = kFootSide * kFootSide * kFootSide;

template <class VX, bool STAGED>
__global__ void __launch_bounds__(512) resample_block_kernel(const int32_t* __restrict__ list, VolumeView src, int srcEntries, size_t srcVoxels, itm_rigid_q q,
                                                             const uint4* __restrict__ dstHash, void* __restrict__ dstVba, size_t dstVoxels, int maxW,
                                                             uint32_t* __restrict__ allocKey, AccelWriter aw) {
  __shared__ long long bases[27];
  __shared__ uint32_t depthTap[STAGED ? kFoot : 1];                               // short: sdf | w_depth << 16; float: the sdf's bits
  __shared__ uint8_t weightTap[STAGED && !VX::kShort ? kFoot : 4];                // float: w_depth
  __shared__ uint32_t colourTap[STAGED && VX::kColor ? kFoot : 1];                // clr[0] | clr[1] << 8 | clr[2] << 16 | w_color << 24
  const int dstSlot = list[blockIdx.x], t = threadIdx.x;
  if (t == 0) allocKey[dstSlot] = 0u;
  const HashEntry de = unpack_entry(dstHash[dstSlot]);
  if (de.ptr < 0 || (size_t)de.ptr * kBlockVoxels + kBlockVoxels > dstVoxels) return;      // swapped out of dst (uniform per workgroup)
  // the base src block of the workgroup: the first voxel its inverse box can touch
  const long long c0[3] = {8ll * de.px, 8ll * de.py, 8ll * de.pz}, c1[3] = {8ll * de.px + 7, 8ll * de.py + 7, 8ll * de.pz + 7};
  long long slo[3], shi[3];
  q30_box(q.inv, q.invT, c0, c1, slo, shi);
  const long long bb[3] = {q30_first(slo[0]) >> 3, q30_first(slo[1]) >> 3, q30_first(slo[2]) >> 3};
  if (t < 27) {
    // (a block beyond the int range cannot exist: fine_block_base refuses what does not fit a short)
    const long long x = bb[0] + t % 3, y = bb[1] + (t / 3) % 3, z = bb[2] + t / 9;
    const bool fits = x >= -32768 && x <= 32767 && y >= -32768 && y <= 32767 && z >= -32768 && z <= 32767;
    bases[t] = fits ? fine_block_base(src, srcEntries, srcVoxels, (int)x, (int)y, (int)z) : -1ll;
  }
  __syncthreads();
  // voxel (vx, vy, vz) of src through the 27 bases; outside them (never, under the row bound) it reads as absent
  auto load_tap = [&](long long vx, long long vy, long long vz) {
    const long long rx = (vx >> 3) - bb[0], ry = (vy >> 3) - bb[1], rz = (vz >> 3) - bb[2];
    typename VX::Reg tap = VX::init();
    if (rx >= 0 && rx < 3 && ry >= 0 && ry < 3 && rz >= 0 && rz < 3) {
      const long long base = bases[(int)rx + 3 * (int)ry + 9 * (int)rz];
      if (base >= 0) tap = VX::load(src.vba, (size_t)base + (size_t)((vx & 7) + ((vy & 7) << 3) + ((vz & 7) << 6)));
    }
    return tap;
  };
  const long long o[3] = {slo[0] >> 30, slo[1] >> 30, slo[2] >> 30};      // the footprint's first voxel
  if constexpr (STAGED) {
    for (int i = t; i < kFoot; i += 512) {
      const typename VX::Reg r = load_tap(o[0] + (i & 15), o[1] + ((i >> 4) & 15), o[2] + (i >> 8));
      if constexpr (VX::kShort) depthTap[i] = rs_first_word(r) & 0x00ffffffu;
      else { depthTap[i] = rs_first_word(r); weightTap[i] = (uint8_t)VX::w_depth(r); }
      if constexpr (VX::kColor) {
        int c[3], wc;
        VX::get_color(r, c, wc);
        colourTap[i] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)wc << 24);
      }
    }
    __syncthreads();
  }
  long long f[3];
  int u[3];
  resample_position(q, c0[0] + (t & 7), c0[1] + ((t >> 3) & 7), c0[2] + (t >> 6), f, u);
  ResampledVoxel<VX> rv;
#pragma unroll
  for (int kz = 0; kz < 2; ++kz)
#pragma unroll
    for (int ky = 0; ky < 2; ++ky)
#pragma unroll
      for (int kx = 0; kx < 2; ++kx) {
        const int c = (kx ? u[0] : 64 - u[0]) * (ky ? u[1] : 64 - u[1]) * (kz ? u[2] : 64 - u[2]);
        const long long vx = f[0] + kx, vy = f[1] + ky, vz = f[2] + kz;
        if constexpr (STAGED) {
          const long long ix = vx - o[0], iy = vy - o[1], iz = vz - o[2];
          if (ix >= 0 && ix < kFootSide && iy >= 0 && iy < kFootSide && iz >= 0 && iz < kFootSide) {      // (always, under the row bound)
            const int i = (int)ix + kFootSide * ((int)iy + kFootSide * (int)iz);
            const uint32_t d = depthTap[i];
            rv.depth(c, d, VX::kShort ? (int)(d >> 16) : (int)weightTap[VX::kShort ? 0 : i]);
            if constexpr (VX::kColor) {
              const uint32_t cw = colourTap[i];
              const int clr[3] = {(int)(cw & 0xffu), (int)((cw >> 8) & 0xffu), (int)((cw >> 16) & 0xffu)};
              rv.colour(c, clr, (int)(cw >> 24));
            }
          } else resample_tap<VX>(rv, c, VX::init());
        } else resample_tap<VX>(rv, c, load_tap(vx, vy, vz));
      }
  const size_t vi = (size_t)de.ptr * kBlockVoxels + t;
  const typename VX::Reg r = combine_voxel<VX>(rv.voxel(), VX::load(dstVba, vi), maxW);
  VX::store(dstVba, vi, r);
  // the block's place in the sdf mirror (the page of a block allocated by this call is mapped here)
  size_t mbase;
  if (aw.block_base_workgroup<true>(de.px, de.py, de.pz, mbase)) aw.store_sdf<VX>(mbase, (uint32_t)t, VX::raw_sdf(r));
}

// dense index: cell i of dst at q = cell + dst's offset, taps through src's array
template <class VX>
__global__ void __launch_bounds__(256) resample_dense_kernel(VolumeView src, itm_rigid_q q, void* __restrict__ dstVba, int dsx, int dsy, int dsz, int dox, int doy, int doz,
                                                             int maxW) {
  const size_t n = (size_t)dsx * (size_t)dsy * (size_t)dsz;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const long long qx = (long long)(i % (size_t)dsx) + dox, qy = (long long)((i / (size_t)dsx) % (size_t)dsy) + doy, qz = (long long)(i / ((size_t)dsx * (size_t)dsy)) + doz;
    long long f[3];
    int u[3];
    resample_position(q, qx, qy, qz, f, u);
    ResampledVoxel<VX> rv;
#pragma unroll
    for (int kz = 0; kz < 2; ++kz)
#pragma unroll
      for (int ky = 0; ky < 2; ++ky)
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
          const int c = (kx ? u[0] : 64 - u[0]) * (ky ? u[1] : 64 - u[1]) * (kz ? u[2] : 64 - u[2]);
          const long long px = f[0] + kx - src.ox, py = f[1] + ky - src.oy, pz = f[2] + kz - src.oz;
          const bool in = px >= 0 && px < src.sx && py >= 0 && py < src.sy && pz >= 0 && pz < src.sz;
          typename VX::Reg tap = VX::init();
          if (in) tap = VX::load(src.vba, (size_t)px + (size_t)py * (size_t)src.sx + (size_t)pz * (size_t)src.sx * (size_t)src.sy);
          resample_tap<VX>(rv, c, tap);
        }
    VX::store(dstVba, i, combine_voxel<VX>(rv.voxel(), VX::load(dstVba, i), maxW));
  }
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_rigid_quantise(const float dstFromSrc[16], float voxelSize, itm_rigid_q* out) {
  if (!dstFromSrc || !out) return set_error(ITM_ERR_INVALID, "rigid quantise: null argument");
  if (!std::isfinite(voxelSize) || !(voxelSize > 0.0f)) return set_error(ITM_ERR_INVALID, "rigid quantise: voxelSize is not a positive finite number");
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(dstFromSrc[i])) return set_error(ITM_ERR_INVALID, "rigid quantise: a non-finite entry");
  if (dstFromSrc[3] != 0.0f || dstFromSrc[7] != 0.0f || dstFromSrc[11] != 0.0f || dstFromSrc[15] != 1.0f)
    return set_error(ITM_ERR_INVALID, "rigid quantise: the bottom row is not (0, 0, 0, 1)");
  double R[3][3], t[3];      // column-major input: R[i][j] = M[4 j + i]
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (double)dstFromSrc[4 * j + i];
    t[i] = (double)dstFromSrc[12 + i];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j] - (i == j ? 1.0 : 0.0);
      if (std::fabs(d) > 1e-4) return set_error(ITM_ERR_INVALID, "rigid quantise: the rotation part is not orthonormal (an entry of R^T R - I above 1e-4)");
    }
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  if (det < 0.0) return set_error(ITM_ERR_INVALID, "rigid quantise: the rotation part is a reflection (det R < 0)");
  // A float matrix is orthonormal to 1e-7 at best, some 50 units of Q30: inv = R^T would then not be the inverse of fwd = R to the
  // precision Q30 is chosen for.  So R is first brought to the rotation next to it, in double: three steps of R <- R (3 I - R^T R) / 2
  // (each squares the distance; a matrix that is orthonormal already -- the identity, the turns by 90 degrees -- stays bit for bit).
  for (int step = 0; step < 3; ++step) {
    double G[3][3], N[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i][j] = (i == j ? 3.0 : 0.0) - (R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j]);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) N[i][j] = 0.5 * (R[i][0] * G[0][j] + R[i][1] * G[1][j] + R[i][2] * G[2][j]);
    memcpy(R, N, sizeof R);
  }
  const double vs = (double)voxelSize, one = 1073741824.0;
  for (int i = 0; i < 3; ++i)
    if (!(std::fabs(t[i]) / vs < 262144.0)) return set_error(ITM_ERR_INVALID, "rigid quantise: the translation is 2^18 voxels or more on an axis");
  itm_rigid_q r;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      r.fwd[3 * i + j] = (int32_t)llrint(R[i][j] * one);
      r.inv[3 * i + j] = (int32_t)llrint(R[j][i] * one);
    }
    r.fwdT[i] = (int64_t)llrint(t[i] / vs * one);
    r.invT[i] = (int64_t)llrint(-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) / vs * one);
  }
  *out = r;
  return ITM_OK;
}

int itm_scene_resample(itm_scene* dst, const itm_scene* src, const itm_rigid_q* q, const int32_t* srcSlots_dev, int n, itm_resample_stats* stats, itm_stream stream) {
  if (dst && src && !q) return set_error(ITM_ERR_INVALID, "scene resample: null transform");      // (second to the null scene)
  { const int rc = check_scene_pair(dst, src, "scene resample", false, true); if (rc) return rc; }
  for (int i = 0; i < 3; ++i) {
    long long rowInv = 0, rowFwd = 0;
    for (int j = 0; j < 3; ++j) { rowInv += llabs((long long)q->inv[3 * i + j]); rowFwd += llabs((long long)q->fwd[3 * i + j]); }
    if (rowInv > kQ30RowBound || rowFwd > kQ30RowBound) return set_error(ITM_ERR_INVALID, "scene resample: a row of the transform sums to more than 1.75 in magnitude");
    if (q->invT[i] <= -kQ30MaxT || q->invT[i] >= kQ30MaxT || q->fwdT[i] <= -kQ30MaxT || q->fwdT[i] >= kQ30MaxT)
      return set_error(ITM_ERR_INVALID, "scene resample: a translation of the transform is 2^18 voxels or more");
  }
  { const int rc = enter_scene_pair(dst, src, srcSlots_dev, n, "scene resample"); if (rc) return rc; }
  const bool hash = dst->cfg.indexType == ITM_INDEX_HASH;
  hipStream_t st = as_stream(stream);
  itm_resample_stats out{};
  VolumeView from = make_volume(src);
  if (!hash)
    return finish_dense(dst, out, &itm_resample_stats::resampled, stats, [&](auto vx) {
      resample_dense_kernel<decltype(vx)><<<4096, 256, 0, st>>>(from, *q, dst->vba, dst->cfg.denseSize[0], dst->cfg.denseSize[1], dst->cfg.denseSize[2], dst->cfg.denseOffset[0],
                                                                dst->cfg.denseOffset[1], dst->cfg.denseOffset[2], dst->prm.maxW);
    });

  // The scratch of a call, kept with dst (scene_ops.h: ResampleArena).  The tail is sized by N, the candidates, known after the count
  // pass: a buffer that has to grow loses its contents, so the count pass then runs once more.
  const int srcChunks = (src->noTotalEntries + kSweepChunk - 1) / kSweepChunk;
  ResampleArena a(kMsCount, (size_t)dst->numChunks, (size_t)srcChunks, (size_t)src->noTotalEntries);
  MergePlacement pl{nullptr, st};
  size_t N = 0;
  void* base = nullptr;
  for (int pass = 0;; ++pass) {
    const size_t need = a.size_tail(N);
    const bool kept = pass > 0 && dst->mergeScratch.get() && need <= dst->mergeScratch.capacity();
    if (kept) break;
    ITM_HIP(dst->mergeScratch.reserve(need));
    base = dst->mergeScratch.get();
    pl.dStats = a.stats.at(base);
    uint8_t* sel = srcSlots_dev ? a.sel.at(base) : nullptr;
    ITM_HIP(hipMemsetAsync(pl.dStats, 0, kMsCount * 4, st));
    if (sel) { const int rc = mark_slots(srcSlots_dev, n, src->noTotalEntries, sel, pl.dStats, st); if (rc) return rc; }
    // (the count pass runs in the same round trip as the mark)
    resample_count_kernel<<<srcChunks, 256, 0, st>>>(src->hash, src->noTotalEntries, sel, *q, a.cnt.at(base), a.chunkCount.at(base), pl.dStats);
    ITM_LAUNCH_CHECK();
    { const int rc = pl.read_stats(); if (rc) return rc; }
    { const int rc = refuse_bad_slots(pl.h, "scene resample"); if (rc) return rc; }      // dst is untouched
    N = (size_t)pl.h[kMsRsCandidates];
  }
  out.considered = pl.h[kMsRsParticipants]; out.srcWithoutBlock = pl.h[kMsRsNoBlock]; out.outOfRange = pl.h[kMsRsOutOfRange]; out.candidates = (int32_t)N;
  // dst's cubes, if nothing has placed them yet: around the block that holds the image of the centre of src's
  place_cubes_like(dst, src, [&](const int c[3], int o[3]) {
    for (int i = 0; i < 3; ++i) {
      const long long v = (long long)q->fwd[3 * i] * (8ll * c[0]) + (long long)q->fwd[3 * i + 1] * (8ll * c[1]) + (long long)q->fwd[3 * i + 2] * (8ll * c[2]) + (long long)q->fwdT[i];
      o[i] = (int)((v >> 30) >> 3);
    }
  });
  if (N == 0) { out.rounds = 1; if (stats) *stats = out; return ITM_OK; }      // (the one round that finds no request)
  pl.where = a.where.at(base); pl.list = a.list.at(base);
  uint4* cand = a.cand.at<uint4>(base);
  resample_fill_kernel<<<srcChunks, 256, 0, st>>>(src->hash, src->noTotalEntries, *q, a.cnt.at(base), a.chunkCount.at(base), srcChunks, (int)N, cand);
  ITM_LAUNCH_CHECK();
  { const int rc = place_positions<0>(dst, cand, (int)N, nullptr, a.chunkCnt.at<int2>(base), st, pl); if (rc) return rc; }
  return finish_placed(dst, pl, out, &itm_resample_stats::resampled, stats,
      [&] { claim_blocks_kernel<<<((int)N + 255) / 256, 256, 0, st>>>((int)N, pl.where, dst->hash, dst->numVoxels, dst->allocKey, pl.list, pl.dStats); },
      [&](auto vx, int count) {
        resample_block_kernel<decltype(vx), ITM_RESAMPLE_STAGED != 0><<<count, 512, 0, st>>>(pl.list, from, src->noTotalEntries, src->numVoxels, *q, dst->hash, dst->vba, dst->numVoxels,
                                                                                             dst->prm.maxW, dst->allocKey, accel_writer(dst));
      });
}

}  // extern "C"
