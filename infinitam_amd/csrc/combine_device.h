// combine_device.h -- the voxel arithmetic of DeviceAgnostic/ITMSwappingEngine.h:7-69 (CombineVoxelInformation) on the register images
// of the codecs, shared by the swapping engine (swapping.hip) and the scene merger (merge.hip).
#pragma once

#include "itm_types.h"

namespace itm {

__device__ inline uint32_t to_uchar_ref(float x) {      // TO_UCHAR3 per component: round half away from zero, then clamp
  int v = (int)((x < 0) ? (x - 0.5f) : (x + 0.5f));
  v = (v < 255) ? v : 255;
  return (uint32_t)((0 < v) ? v : 0);
}
template <class VX>
__device__ inline typename VX::Reg combine_voxel(typename VX::Reg src, typename VX::Reg dst, int maxW) {
  {
    int newW = VX::w_depth(dst);
    const int oldW = VX::w_depth(src);
    float newF = VX::kShort ? VX::raw_sdf(dst) / 32767.0f : VX::raw_sdf(dst);
    const float oldF = VX::kShort ? VX::raw_sdf(src) / 32767.0f : VX::raw_sdf(src);
    if (oldW != 0) {
      newF = (float)oldW * oldF + (float)newW * newF;
      newW = oldW + newW;
      newF /= (float)newW;
      newW = (newW < maxW) ? newW : maxW;
      dst = VX::with_depth(dst, newF, newW);
    }
  }
  if constexpr (VX::kColor) {
    int nc[3], oc[3], newW, oldW;
    VX::get_color(dst, nc, newW);
    VX::get_color(src, oc, oldW);
    if (oldW != 0) {
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float newC = (float)nc[k] / 255.0f, oldC = (float)oc[k] / 255.0f;
        c[k] = oldC * (float)oldW + newC * (float)newW;
      }
      newW = oldW + newW;
#pragma unroll
      for (int k = 0; k < 3; ++k) { c[k] /= (float)newW; nc[k] = (int)to_uchar_ref(c[k] * 255.0f); }
      newW = (newW < maxW) ? newW : maxW;
      dst = VX::with_color(dst, nc, newW & 0xff);
    }
  }
  return dst;
}

}  // namespace itm
