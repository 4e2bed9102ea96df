// fuse_device.h -- the per-voxel fusion arithmetic shared by the hash engine (integrate.hip) and the dense engine (integrate_dense.hip).
//
// Reference behaviour:
//   computeUpdatedVoxelDepthInfo / ColorInfo / ComputeUpdatedVoxelInfo
//                               DeviceAgnostic/ITMSceneReconstructionEngine.h:9-139
//   interpolateBilinear         DeviceAgnostic/ITMPixelUtils.h:11-39
#pragma once
#include "itm_internal.h"

namespace itm {

struct FuseParams {
  Mat4 M_d, M_rgb;
  float fx, fy, cx, cy;
  float fxc, fyc, cxc, cyc;
  float mu, voxelSize;
  float rcpMu;      // RN(1/mu), computed on the host
  int muFast;       // 1: eta/mu may use the 3-instruction reciprocal division (host-checked)
  int maxW;
  int W, H, Wc, Hc;
  int stopAtMax;
  AccelOrigin org;  // where the sdf mirror cube lies (hash scenes)
  int idsCap;       // capacity of the visible list (ids), for the speculative first fetch of integrate_hash_body
};

// Depth part, stage 1: project the voxel; returns the index of the depth pixel it falls on, or -1 when the voxel
// cannot be touched (behind the camera / outside the image).  Operation order as SURVEY.md Appendix A.5.
// EARLY_OUT: the conservative frustum test in front of the divisions.  It pays where most voxels leave through it (a dense volume: ~70 %
// of the voxels are outside the image) and costs four products and four comparisons per voxel where hardly any does (the blocks of a
// visible list: the hash kernels run without it -- round 6, ~10 % of their vector instructions).
// IN_RANGE: the caller has shown that pc.z lies in [1e-4, 1e4] (integrate_item decides it once for all voxels of its item): neither the
// pc.z <= 0 exit nor the IEEE-division side is compiled in; the arithmetic that remains is the other form's, operation for operation.
template <bool EARLY_OUT = true, bool IN_RANGE = false>
__device__ inline int fuse_depth_project(float mx, float my, float mz, const FuseParams& p, float& pcz) {
  Vec3 pc = transform_point(p.M_d, mx, my, mz);
  pcz = pc.z;
  if constexpr (!IN_RANGE) {
    if (pc.z <= 0) return -1;
  }
  const float tx = p.fx * pc.x, ty = p.fy * pc.y;
#if ITM_FAST_DIVISIONS
  // Conservative early-out before the two divisions: the voxel is rejected below when
  // u = tx/z + cx is outside [1, W-2]; half a pixel of margin dwarfs every rounding error, so this
  // never rejects a voxel the exact test would keep (most voxels of a dense volume leave here).
  if constexpr (EARLY_OUT) {
    if (tx < (0.5f - p.cx) * pc.z || tx > ((float)(p.W - 2) + 0.5f - p.cx) * pc.z ||
        ty < (0.5f - p.cy) * pc.z || ty > ((float)(p.H - 2) + 0.5f - p.cy) * pc.z) return -1;
  }
  float u, v;
  if (IN_RANGE || (pc.z >= 1e-4f && pc.z <= 1e4f)) {       // normal range: shared refined reciprocal, exact quotients
    const float rz = refined_rcp(pc.z);
    u = div_by_rcp(tx, pc.z, rz) + p.cx;
    v = div_by_rcp(ty, pc.z, rz) + p.cy;
  } else {
    u = tx / pc.z + p.cx;
    v = ty / pc.z + p.cy;
  }
#else
  const float u = tx / pc.z + p.cx;
  const float v = ty / pc.z + p.cy;
#endif
  if ((u < 1) || (u > p.W - 2) || (v < 1) || (v > p.H - 2)) return -1;
  // (both factors are below 2^23 -- images have fewer than 2^24 pixels, scene.hip -- so the 24-bit multiply-add is exact and one
  // full-rate instruction where the 32-bit form is a quarter-rate 64-bit mad)
  return __mul24((int)(v + 0.5f), p.W) + (int)(u + 0.5f);
}

// The running average of computeUpdatedVoxelDepthInfo (DeviceAgnostic/ITMSceneReconstructionEngine.h:45-55) with the clamped
// observation newF = MIN(1, eta / mu).
template <class VX>
__device__ inline void fuse_average(typename VX::Reg& r, float newF, const FuseParams& p) {
  const float oldF = VX::to_float(VX::raw_sdf(r));
  const int oldW = VX::w_depth(r);
  int newW = 1;
  newF = (float)oldW * oldF + (float)newW * newF;
  newW = oldW + newW;
#if ITM_FAST_DIVISIONS
  {
    // newW is an integer in [1, 256]: the refined reciprocal equals RN(1/newW) for all of them (tested),
    // its significand is never all ones, so the 3-instruction quotient is the correctly rounded one
    const float w = (float)newW;
    newF = div_markstein(newF, w, refined_rcp(w));
  }
#else
  newF /= (float)newW;
#endif
  newW = (newW < p.maxW) ? newW : p.maxW;
  r = VX::with_depth(r, newF, newW);
}

// Stage 2: the running average with the measured depth dm of that pixel.  Returns eta (or -1 when the voxel is not
// touched); `touched` tells whether the register image changed.
template <class VX>
__device__ inline float fuse_depth_update(typename VX::Reg& r, float dm, float pcz, const FuseParams& p, bool& touched) {
  if (dm <= 0.0f) return -1;
  const float eta = dm - pcz;
  if (eta < -p.mu) return eta;
#if ITM_FAST_DIVISIONS
  float newF = p.muFast ? div_markstein(eta, p.mu, p.rcpMu) : eta / p.mu;
#else
  float newF = eta / p.mu;
#endif
  newF = (1.0f < newF) ? 1.0f : newF;
  fuse_average<VX>(r, newF, p);
  touched = true;
  return eta;
}

template <class VX>
__device__ inline float fuse_depth(typename VX::Reg& r, float mx, float my, float mz, const float* __restrict__ depth,
                                   const FuseParams& p, bool& touched) {
  float pcz;
  const int pix = fuse_depth_project(mx, my, mz, p, pcz);
  if (pix < 0) return -1;
  return fuse_depth_update<VX>(r, depth[pix], pcz, p, touched);
}

// The colour update's condition, !(eta > mu || fabs(eta / mu) > 0.25) (DeviceAgnostic/ITMSceneReconstructionEngine.h:127-131), without the
// IEEE division macro on the common path: for eta < -mu the correctly rounded quotient is <= -1 (division is monotone), so the voxel
// is outside the band whatever eta is (-inf included); for eta in [-mu, mu] the Markstein quotient is the correctly rounded one
// whenever it is a normal number, and both are far below 0.25 when it is not; a NaN eta passes every comparison as it does in the
// reference.  (Round 6: ~10 vector instructions less per voxel of the colour kernels.)
__device__ inline bool in_colour_band(float eta, const FuseParams& p) {
  if (eta < -p.mu || eta > p.mu) return false;
#if ITM_FAST_DIVISIONS
  const float q = p.muFast ? div_markstein(eta, p.mu, p.rcpMu) : eta / p.mu;
#else
  const float q = eta / p.mu;
#endif
  return !(fabsf(q) > 0.25f);
}

__device__ inline float round_half_away(float x) { return (x < 0) ? (x - 0.5f) : (x + 0.5f); }

template <class VX>
__device__ inline void fuse_colour(typename VX::Reg& r, float mx, float my, float mz, const uchar4* __restrict__ rgb, const FuseParams& p) {
  int oc[3], owc;
  VX::get_color(r, oc, owc);
  const float oldW = (float)owc;
  Vec3 pc = transform_point(p.M_rgb, mx, my, mz);
  float u, v;
#if ITM_FAST_DIVISIONS
  if (pc.z >= 1e-4f && pc.z <= 1e4f) {       // normal range: shared refined reciprocal, exact quotients (as in fuse_depth)
    const float rz = refined_rcp(pc.z);
    u = div_by_rcp(p.fxc * pc.x, pc.z, rz) + p.cxc;
    v = div_by_rcp(p.fyc * pc.y, pc.z, rz) + p.cyc;
  } else
#endif
  {
    u = p.fxc * pc.x / pc.z + p.cxc;
    v = p.fyc * pc.y / pc.z + p.cyc;
  }
  if ((u < 1) || (u > p.Wc - 2) || (v < 1) || (v > p.Hc - 2)) return;
  const int px = (int)floorf(u), py = (int)floorf(v);
  const float dx = u - (float)px, dy = v - (float)py;
  // interpolateBilinear (DeviceAgnostic/ITMPixelUtils.h:11-39) fetches b, c, d only when their weight is not zero and uses 0 otherwise.
  // All four taps are inside the image here (1 <= u <= Wc - 2, 1 <= v <= Hc - 2), and a finite channel value times a zero weight is
  // the same +0 the reference adds: fetching the four unconditionally is bit-identical and ONE round trip instead of three
  // dependent ones (until round 6 each conditional tap sat in its own branch behind a wait of its own).
  const uchar4* __restrict__ row = rgb + (size_t)py * p.Wc + px;
  const uchar4 A = row[0], B = row[1], C = row[p.Wc], D = row[p.Wc + 1];
  const float a4[3] = {(float)A.x, (float)A.y, (float)A.z}, b4[3] = {(float)B.x, (float)B.y, (float)B.z};
  const float c4[3] = {(float)C.x, (float)C.y, (float)C.z}, d4[3] = {(float)D.x, (float)D.y, (float)D.z};
  float newW = oldW + 1.0f;
  int nc[3];
#if ITM_FAST_DIVISIONS
  // x / 255 and c / newW (newW an integer in [1, 256]) as Markstein quotients: RN(1/255) is a compile-time constant,
  // the refined reciprocal equals RN(1/newW) for every such weight, neither significand is all ones
  // (tests/test_hip_parity.py::test_fast_divisions_are_ieee, cases 5 and 6)
  const float r255 = 1.0f / 255.0f;
  const float rW = refined_rcp(newW);
#endif
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float m = (a4[k] * (1.0f - dx) * (1.0f - dy) + b4[k] * dx * (1.0f - dy) + c4[k] * (1.0f - dx) * dy + d4[k] * dx * dy);
#if ITM_FAST_DIVISIONS
    m = div_markstein(m, 255.0f, r255);
    float c = div_markstein((float)oc[k], 255.0f, r255) * oldW + m * 1.0f;
    c = div_markstein(c, newW, rW);
#else
    m = m / 255.0f;
    float c = ((float)oc[k] / 255.0f) * oldW + m * 1.0f;
    c /= newW;
#endif
    int vi = (int)round_half_away(c * 255.0f);
    vi = (vi < 255) ? vi : 255;
    nc[k] = (0 < vi) ? vi : 0;
  }
  const float maxWf = (float)(p.maxW & 0xff);
  newW = (newW < maxWf) ? newW : maxWf;
  r = VX::with_color(r, nc, (int)newW);
}

// ---- the inverse update (itm_deintegrate_from_scene, deintegrate.hip; include/itm_hip.h states the definition) -------------------------
// What became of one voxel, as bits: the statistics are counts of them.
enum : uint32_t { kUnfuseTouched = 1u, kUnfuseReset = 2u, kUnfuseUnobserved = 4u, kUnfuseSaturated = 8u, kUnfuseClamped = 16u,
                  kUnfuseColoured = 32u, kUnfuseColourReset = 64u };

// Kept as it is by keepSaturated: the voxel may have absorbed any number of observations since its weight reached maxW.
template <class VX>
__device__ inline bool unfuse_kept(const typename VX::Reg& r, const FuseParams& p, int keepSaturated) {
  const int w = VX::w_depth(r);
  return keepSaturated && w != 0 && w >= p.maxW;      // (weight 0 is "unobserved" whatever maxW is)
}

// fuse_average backwards: the observation obs = MIN(1, eta / mu) leaves the running average of a voxel that is not unfuse_kept.
// Returns the kUnfuse* bits of the depth part.
template <class VX>
__device__ inline uint32_t unfuse_average(typename VX::Reg& r, float obs) {
  const int oldW = VX::w_depth(r);
  if (oldW == 0) return kUnfuseUnobserved;
  if (oldW == 1) {
    r = VX::with_depth(r, 1.0f, 0);      // SDF_initialValue(): 32767 / 1.0f
    return kUnfuseTouched | kUnfuseReset;
  }
  const float oldF = VX::to_float(VX::raw_sdf(r));
  float f = (float)oldW * oldF;
  f = f - obs;
  const float w = (float)(oldW - 1);
#if ITM_FAST_DIVISIONS
  // oldW - 1 is an integer in [1, 254]: inside the set fuse_average divides by, for which the refined reciprocal is RN(1 / w) (tested)
  f = div_markstein(f, w, refined_rcp(w));
#else
  f /= w;
#endif
  // removing an observation that was never added can leave [-1, 1], which the short encoding cannot hold
  const float c = (1.0f < f) ? 1.0f : f;        // MIN(1.0f, f)
  const float g = (-1.0f < c) ? c : -1.0f;      // MAX(-1.0f, c)
  const uint32_t clamped = (g != f) ? kUnfuseClamped : 0u;
  r = VX::with_depth(r, g, oldW - 1);
  return kUnfuseTouched | clamped;
}

// Stage 2 of the depth part, the exits of fuse_depth_update operation for operation.  Returns eta (or -1 when the voxel is not touched).
template <class VX>
__device__ inline float unfuse_depth_update(typename VX::Reg& r, float dm, float pcz, const FuseParams& p, uint32_t& what) {
  if (dm <= 0.0f) return -1;
  const float eta = dm - pcz;
  if (eta < -p.mu) return eta;
#if ITM_FAST_DIVISIONS
  float obs = p.muFast ? div_markstein(eta, p.mu, p.rcpMu) : eta / p.mu;
#else
  float obs = eta / p.mu;
#endif
  obs = (1.0f < obs) ? 1.0f : obs;
  what |= unfuse_average<VX>(r, obs);
  return eta;
}

// fuse_colour backwards: the projection, the image bounds and the bilinear colour are fuse_colour's, operation for operation.
// Returns the kUnfuse* bits of the colour part.
template <class VX>
__device__ inline uint32_t unfuse_colour(typename VX::Reg& r, float mx, float my, float mz, const uchar4* __restrict__ rgb, const FuseParams& p, int keepSaturated) {
  int oc[3], owc;
  VX::get_color(r, oc, owc);
  if (owc == 0 || (keepSaturated && owc >= (p.maxW & 0xff))) return 0u;
  Vec3 pc = transform_point(p.M_rgb, mx, my, mz);
  float u, v;
#if ITM_FAST_DIVISIONS
  if (pc.z >= 1e-4f && pc.z <= 1e4f) {
    const float rz = refined_rcp(pc.z);
    u = div_by_rcp(p.fxc * pc.x, pc.z, rz) + p.cxc;
    v = div_by_rcp(p.fyc * pc.y, pc.z, rz) + p.cyc;
  } else
#endif
  {
    u = p.fxc * pc.x / pc.z + p.cxc;
    v = p.fyc * pc.y / pc.z + p.cyc;
  }
  if ((u < 1) || (u > p.Wc - 2) || (v < 1) || (v > p.Hc - 2)) return 0u;
  int nc[3] = {0, 0, 0};
  if (owc == 1) {
    r = VX::with_color(r, nc, 0);
    return kUnfuseColoured | kUnfuseColourReset;
  }
  const int px = (int)floorf(u), py = (int)floorf(v);
  const float dx = u - (float)px, dy = v - (float)py;
  const uchar4* __restrict__ row = rgb + (size_t)py * p.Wc + px;
  const uchar4 A = row[0], B = row[1], C = row[p.Wc], D = row[p.Wc + 1];      // (all four taps: see fuse_colour)
  const float a4[3] = {(float)A.x, (float)A.y, (float)A.z}, b4[3] = {(float)B.x, (float)B.y, (float)B.z};
  const float c4[3] = {(float)C.x, (float)C.y, (float)C.z}, d4[3] = {(float)D.x, (float)D.y, (float)D.z};
  const float oldW = (float)owc, newW = oldW - 1.0f;      // newW: an integer in [1, 254]
#if ITM_FAST_DIVISIONS
  const float r255 = 1.0f / 255.0f;
  const float rW = refined_rcp(newW);
#endif
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float m = (a4[k] * (1.0f - dx) * (1.0f - dy) + b4[k] * dx * (1.0f - dy) + c4[k] * (1.0f - dx) * dy + d4[k] * dx * dy);
#if ITM_FAST_DIVISIONS
    m = div_markstein(m, 255.0f, r255);
    float c = div_markstein((float)oc[k], 255.0f, r255) * oldW;
    c = c - m;
    c = div_markstein(c, newW, rW);
#else
    m = m / 255.0f;
    float c = ((float)oc[k] / 255.0f) * oldW;
    c = c - m;
    c /= newW;
#endif
    int vi = (int)round_half_away(c * 255.0f);
    vi = (vi < 255) ? vi : 255;
    nc[k] = (0 < vi) ? vi : 0;
  }
  r = VX::with_color(r, nc, owc - 1);
  return kUnfuseColoured;
}

// One voxel whole (the dense kernel; the hash kernel stages the same calls over the slices of an item).  Returns the kUnfuse* bits.
template <class VX>
__device__ inline uint32_t unfuse_voxel(typename VX::Reg& r, float mx, float my, float mz, const float* __restrict__ depth,
                                        const uchar4* __restrict__ rgb, const FuseParams& p, int keepSaturated) {
  float pcz;
  const int pix = fuse_depth_project(mx, my, mz, p, pcz);
  const float dm = (pix >= 0) ? depth[pix] : 0.0f;
  // (a kept voxel is skipped altogether, colour included; it counts where the depth part would have written it)
  if (unfuse_kept<VX>(r, p, keepSaturated)) return (dm <= 0.0f || dm - pcz < -p.mu) ? 0u : kUnfuseSaturated;
  uint32_t what = 0u;
  const float eta = (pix >= 0) ? unfuse_depth_update<VX>(r, dm, pcz, p, what) : -1.0f;
  if constexpr (VX::kColor) {
    if (in_colour_band(eta, p)) what |= unfuse_colour<VX>(r, mx, my, mz, rgb, p, keepSaturated);
  }
  return what;
}

template <class VX>
__device__ inline bool fuse_voxel(typename VX::Reg& r, float mx, float my, float mz, const float* __restrict__ depth,
                                  const uchar4* __restrict__ rgb, const FuseParams& p) {
  bool touched = false;
  const float eta = fuse_depth<VX>(r, mx, my, mz, depth, p, touched);
  if constexpr (VX::kColor) {
    if (in_colour_band(eta, p)) {
      fuse_colour<VX>(r, mx, my, mz, rgb, p);
      touched = true;
    }
  }
  return touched;
}

}  // namespace itm
