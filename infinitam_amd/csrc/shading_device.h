// shading_device.h -- per-pixel shading helpers shared by the visualisation kernels.
//
// Reference behaviour restated:
//   drawPixelGrey / computeNormalAndAngle (both variants)  DeviceAgnostic/ITMVisualisationEngine.h:175-260
//   computeSingleNormalFromSDF / readFromSDF_color4u_interpolated  DeviceAgnostic/ITMRepresentationAccess.h:187-337
#pragma once

#include <cstring>

#include "itm_internal.h"
#include "raycast_device.h"
#include "sample_device.h"

namespace itm {

static inline void make_ray_params(const itm_scene* s, const float* invM, const float* intr, int W, int H, RayParams& p) {
  memcpy(p.invM.m, invM, 64);
  p.ifx = 1.0f / intr[0]; p.ify = 1.0f / intr[1]; p.cx = intr[2]; p.cy = intr[3];
  p.oneOverVoxel = 1.0f / s->prm.voxelSize;
  p.mu = s->prm.mu; p.voxelSize = s->prm.voxelSize;
  p.lx = -invM[8]; p.ly = -invM[9]; p.lz = -invM[10];
  p.W = W; p.H = H;
}

__device__ inline uchar4 grey_pixel(float angle) {  // drawPixelGrey
  const float o = (0.8f * angle + 0.2f) * 255.0f;
  const unsigned char g = (unsigned char)o;
  return make_uchar4(g, g, g, g);
}

// computeNormalAndAngle<useSmoothing = true> (DeviceAgnostic/ITMVisualisationEngine.h:191-254); `at(x, y)` returns the ray-cast result of a pixel
template <class AT>
__device__ inline bool normal_from_hits_at(AT&& at, int x, int y, int W, int H, float voxelSize,
                                           float lx, float ly, float lz, float& nx, float& ny, float& nz, float& angle) {
  if (y <= 2 || y >= H - 3 || x <= 2 || x >= W - 3) return false;
  float4 xp = at(x + 2, y), yp = at(x, y + 2);
  float4 xm = at(x - 2, y), ym = at(x, y - 2);
  float dxx = 0, dxy = 0, dxz = 0, dyx = 0, dyy = 0, dyz = 0;
  bool plus1 = false;
  if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) plus1 = true;
  else {
    dxx = xp.x - xm.x; dxy = xp.y - xm.y; dxz = xp.z - xm.z;
    dyx = yp.x - ym.x; dyy = yp.y - ym.y; dyz = yp.z - ym.z;
    const float a = dxx * dxx + dxy * dxy + dxz * dxz, b = dyx * dyx + dyy * dyy + dyz * dyz;
    const float l = (a < b) ? b : a;
    if (l * voxelSize * voxelSize > (0.15f * 0.15f)) plus1 = true;
  }
  if (plus1) {
    xp = at(x + 1, y); yp = at(x, y + 1);
    xm = at(x - 1, y); ym = at(x, y - 1);
    dxx = xp.x - xm.x; dxy = xp.y - xm.y; dxz = xp.z - xm.z;
    dyx = yp.x - ym.x; dyy = yp.y - ym.y; dyz = yp.z - ym.z;
    if (xp.w <= 0 || yp.w <= 0 || xm.w <= 0 || ym.w <= 0) return false;
  }
  nx = -(dxy * dyz - dxz * dyy);
  ny = -(dxz * dyx - dxx * dyz);
  nz = -(dxx * dyy - dxy * dyx);
  const float sc = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
  nx *= sc; ny *= sc; nz *= sc;
  angle = nx * lx + ny * ly + nz * lz;
  return angle > 0.0f;
}
__device__ inline bool normal_from_hits(const float4* __restrict__ rays, int x, int y, int W, int H, float voxelSize,
                                        float lx, float ly, float lz, float& nx, float& ny, float& nz, float& angle) {
  return normal_from_hits_at([&](int qx, int qy) { return rays[qx + qy * W]; }, x, y, W, H, voxelSize, lx, ly, lz, nx, ny, nz, angle);
}

template <class VX, bool DENSE>
__device__ inline float raw_at(const VolumeView& vol, int x, int y, int z) {
  BlockCache c; bool f;   // computeSingleNormalFromSDF uses the uncached readVoxel overload
  return read_raw_sdf<VX, DENSE>(vol, x, y, z, f, c);
}

// computeSingleNormalFromSDF at a point of the volume: gradient_axis (sample_device.h) over the uncached reads -- a fresh BlockCache per
// voxel (raw_at), as the reference's readVoxel overload there.  (The functor captures by reference: by value the compiler hoists the
// view's loads over the cover tests of the hash path, 160 registers instead of 98 and the mesh attributes a third slower)
template <class VX, bool DENSE>
__device__ inline void sdf_gradient(const VolumeView& vol, float px, float py, float pz, float& gx, float& gy, float& gz) {
  const float bx = floorf(px), by = floorf(py), bz = floorf(pz);
  const float fx = px - bx, fy = py - by, fz = pz - bz;
  const int ix = (int)bx, iy = (int)by, iz = (int)bz;
  auto raw = [&](int dx, int dy, int dz) { return raw_at<VX, DENSE>(vol, ix + dx, iy + dy, iz + dz); };
  gx = gradient_axis<VX, 0>(raw, fx, fy, fz);
  gy = gradient_axis<VX, 1>(raw, fy, fx, fz);
  gz = gradient_axis<VX, 2>(raw, fz, fx, fy);
}

template <class VX, bool DENSE>
__device__ inline bool normal_from_sdf(const VolumeView& vol, float px, float py, float pz, const RayParams& p,
                                       float& nx, float& ny, float& nz, float& angle) {
  sdf_gradient<VX, DENSE>(vol, px, py, pz, nx, ny, nz);
  const float sc = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);
  nx *= sc; ny *= sc; nz *= sc;
  angle = nx * p.lx + ny * p.ly + nz * p.lz;
  return angle > 0.0f;
}

// readFromSDF_color4u_interpolated at a point of the volume; returns (r,g,b)/255 and w = 1: colour_from (sample_device.h) over the voxels,
// one block cache carried across the eight taps
template <class VX, bool DENSE>
__device__ inline float4 colour_at(const VolumeView& vol, float px, float py, float pz) {
  if constexpr (!VX::kColor) {
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    BlockCache cache;
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
    auto packed = [&](int dx, int dy, int dz) {
      const long long a = locate_voxel<DENSE>(vol, ix + dx, iy + dy, iz + dz, cache);
      int c[3] = {0, 0, 0}, wc = 0;
      if (a >= 0) VX::get_color(VX::load(vol.vba, (size_t)a), c, wc);
      return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
    };
    return colour_from(packed, px - flx, py - fly, pz - flz);
  }
}

}  // namespace itm
