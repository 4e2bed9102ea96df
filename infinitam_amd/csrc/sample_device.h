// sample_device.h -- the reference's per-point samplers over ANY source of voxel values, the only statement of their arithmetic: the
// callers fetch the neighbourhood their own way (the volume voxel by voxel: shading_device.h; LDS planes of a block: mesh_attributes.hip;
// one gather per query point: query.hip) and hand it over as a functor.
//
// Reference behaviour restated:
//   computeSingleNormalFromSDF            DeviceAgnostic/ITMRepresentationAccess.h:224-337
//   readFromSDF_color4u_interpolated      DeviceAgnostic/ITMRepresentationAccess.h:187-222
//   drawPixelColour (float -> uchar)      DeviceAgnostic/ITMVisualisationEngine.h:270-279
#pragma once

#include "itm_types.h"

namespace itm {

// One component of the sdf gradient at a fractional position over any source of raw sdf values: `raw(dx, dy, dz)` is the voxel at
// floor(p) + (dx, dy, dz).  Along AXIS the volume is sampled on the four integer planes k = -1, 0, 1, 2 around the position, each plane
// blended bilinearly over the other two axes (u, v: the remaining axes in x < y < z order); the component is the difference between the
// linear blends of planes (1, 2) and of planes (0, -1).  The products and sums are the reference's, term for term:
//   plane = s00 (1-fu)(1-fv) + s10 fu (1-fv) + s01 (1-fu) fv + s11 fu fv,   lower = plane0 fa + plane-1 (1-fa),   upper = plane1 (1-fa) + plane2 fa
template <class VX, int AXIS, class S>
__device__ inline float gradient_axis(S&& raw, float fa, float fu, float fv) {
  auto sample = [&](int k, int u, int v) {
    const int dx = (AXIS == 0) ? k : u;
    const int dy = (AXIS == 1) ? k : (AXIS == 0 ? u : v);
    const int dz = (AXIS == 2) ? k : v;
    return raw(dx, dy, dz);
  };
  const float gu = 1.0f - fu, gv = 1.0f - fv, ga = 1.0f - fa;
  float plane[4];
#pragma unroll
  for (int k = -1; k <= 2; ++k)
    plane[k + 1] = sample(k, 0, 0) * gu * gv + sample(k, 1, 0) * fu * gv + sample(k, 0, 1) * gu * fv + sample(k, 1, 1) * fu * fv;
  const float lower = plane[1] * fa + plane[0] * ga;
  return VX::to_float(plane[2] * ga + plane[3] * fa - lower);
}

// The derivative of the trilinear interpolant itself (Corners::trilinear, volume_device.h) from the same eight raw corner values
// v[dx + 2 dy + 4 dz] and fractions (cx, cy, cz), per voxel: what a solver that minimises the interpolated sdf differentiates (the
// 32-tap gradient above is the reference's shading normal: a different function, and it reads defaults beside the band).  Along an axis
// the four differences of the cell's edges parallel to it are blended bilinearly with the other two fractions, the first of them
// innermost; every product and sum is rounded on its own:
//   g[0] = (1-cz) ((1-cy) (v1-v0) + cy (v3-v2)) + cz ((1-cy) (v5-v4) + cy (v7-v6))
//   g[1] = (1-cz) ((1-cx) (v2-v0) + cx (v3-v1)) + cz ((1-cx) (v6-v4) + cx (v7-v5))
//   g[2] = (1-cy) ((1-cx) (v4-v0) + cx (v5-v1)) + cy ((1-cx) (v6-v2) + cx (v7-v3))
// each blended on raw values and then converted, as the value is.
template <class VX>
__device__ inline void trilinear_gradient(const float v[8], float cx, float cy, float cz, float g[3]) {
  const float gx = 1.0f - cx, gy = 1.0f - cy, gz = 1.0f - cz;
  g[0] = VX::to_float(gz * (gy * (v[1] - v[0]) + cy * (v[3] - v[2])) + cz * (gy * (v[5] - v[4]) + cy * (v[7] - v[6])));
  g[1] = VX::to_float(gz * (gx * (v[2] - v[0]) + cx * (v[3] - v[1])) + cz * (gx * (v[6] - v[4]) + cx * (v[7] - v[5])));
  g[2] = VX::to_float(gy * (gx * (v[4] - v[0]) + cx * (v[5] - v[1])) + cy * (gx * (v[6] - v[2]) + cx * (v[7] - v[3])));
}

// The colour at a fractional position (cx, cy, cz: its fractions) over any source of packed colours: `packed(dx, dy, dz)` is the voxel at
// floor(p) + (dx, dy, dz) as r | g << 8 | b << 16, 0 where no voxel is stored.  Returns (r, g, b) / 255 and w = 1.
template <class C>
__device__ inline float4 colour_from(C&& packed, float cx, float cy, float cz) {
  float r[3] = {0.0f, 0.0f, 0.0f};
  auto add = [&](int dx, int dy, int dz, float wgt) {
    const uint32_t c = packed(dx, dy, dz);
    r[0] += wgt * (float)(int)(c & 0xffu); r[1] += wgt * (float)(int)((c >> 8) & 0xffu); r[2] += wgt * (float)(int)((c >> 16) & 0xffu);
  };
  add(0, 0, 0, (1.0f - cx) * (1.0f - cy) * (1.0f - cz));
  add(1, 0, 0, (cx) * (1.0f - cy) * (1.0f - cz));
  add(0, 1, 0, (1.0f - cx) * (cy) * (1.0f - cz));
  add(1, 1, 0, (cx) * (cy) * (1.0f - cz));
  add(0, 0, 1, (1.0f - cx) * (1.0f - cy) * cz);
  add(1, 0, 1, (cx) * (1.0f - cy) * cz);
  add(0, 1, 1, (1.0f - cx) * (cy)*cz);
  add(1, 1, 1, (cx) * (cy)*cz);
  return make_float4(r[0] / 255.0f, r[1] / 255.0f, r[2] / 255.0f, 255.0f / 255.0f);
}

__device__ inline void store_normal(float* __restrict__ o, float gx, float gy, float gz) {
  const float sc = 1.0f / sqrtf(gx * gx + gy * gy + gz * gz);
  float nx = gx * sc, ny = gy * sc, nz = gz * sc;
  if (!(__builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz))) nx = ny = nz = 0.0f;   // zero or overflowing length
  o[0] = nx; o[1] = ny; o[2] = nz;
}

__device__ inline uchar4 colour_bytes(float4 c) {   // drawPixelColour
  return make_uchar4((unsigned char)(c.x * 255.0f), (unsigned char)(c.y * 255.0f), (unsigned char)(c.z * 255.0f), 255);
}

}  // namespace itm
