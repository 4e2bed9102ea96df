// integrate_dense.hip -- IntegrateIntoScene for ITMPlainVoxelArray volumes (the per-voxel arithmetic is fuse_device.h's).
//
// Reference behaviour:
//   IntegrateIntoScene (dense)  DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:319-369
//
// MI355X design: the ITMVoxel_s kernels stream the volume with 16-byte accesses (4 ITMVoxel_s per lane), cull whole columns of groups
// against the frustum with two integer comparisons, classify groups against min / max tiles of the depth image and write only 128-bit
// groups that changed.  The depth map is small (1.2 MB) and stays in L2.  Every other voxel type takes one voxel per lane.
#include <cmath>
#include <cstring>

#include "fuse_device.h"

namespace itm {


// Dense volume, generic voxel type: one voxel per lane, x fastest (coalesced).
template <class VX>
__global__ void __launch_bounds__(256) integrate_dense_kernel(void* __restrict__ vba, const float* __restrict__ depth,
                                                              const uchar4* __restrict__ rgb, FuseParams p, int sx, int sy, int sz,
                                                              int ox, int oy, int oz) {
  const size_t n = (size_t)sx * sy * sz;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t loc = (size_t)blockIdx.x * blockDim.x + threadIdx.x; loc < n; loc += stride) {
    const int z = (int)(loc / ((size_t)sx * sy));
    const int rem = (int)(loc - (size_t)z * sx * sy);
    const int y = rem / sx;
    const int x = rem - y * sx;
    typename VX::Reg r = VX::load(vba, loc);
    if (p.stopAtMax && VX::w_depth(r) == p.maxW) continue;
    const float mx = (float)(x + ox) * p.voxelSize, my = (float)(y + oy) * p.voxelSize, mz = (float)(z + oz) * p.voxelSize;
    if (fuse_voxel<VX>(r, mx, my, mz, depth, rgb, p)) VX::store(vba, loc, r);
  }
}

// ---- depth tiles: min / max of the depth image over tiles of 8, 16, 32 and 64 pixels ------------------------------------------
// Most voxels a dense volume presents to a frame lie in observed free space (eta >= mu: the observation is clamped to exactly 1)
// or in the shadow of a surface (eta < -mu: the voxel is not touched).  For a 4-voxel group whose whole pixel footprint falls into
// tiles with  min depth - max pc.z >= mu  (resp.  max depth - min pc.z < -mu)  every voxel of the group takes that branch of
// computeUpdatedVoxelDepthInfo, so neither the projection with its two divisions nor the depth gathers are needed: the free-space
// update is the running average with newF = 1 (for a voxel still holding the initial 32767 simply w + 1), the shadow group is not
// even fetched.  The bounds are conservative (one and a half pixels and 1e-5 of the coordinate magnitudes of slack, two orders above
// the rounding of the exact path), so the result is the exact path's, bit for bit; tests/test_dense_cull.py runs the classified
// kernel against the exact one over whole volumes and checks every classified group against the exact per-voxel outcome
// (itm_debug_dense_classify_check).
constexpr int kTileLevels = 4;       // tile sides 8, 16, 32, 64
struct TileLevels {
  int off[kTileLevels], tw[kTileLevels], th[kTileLevels];
  int total;
};
static TileLevels tile_levels(int w, int h) {
  TileLevels t; int o = 0;
  for (int l = 0; l < kTileLevels; ++l) {
    const int side = 8 << l;
    t.off[l] = o; t.tw[l] = (w + side - 1) / side; t.th[l] = (h + side - 1) / side;
    o += t.tw[l] * t.th[l];
  }
  t.total = o;
  return t;
}
// One workgroup per 64 x 64 pixels: lane <-> a 4 x 4 patch, LDS reduction to the 8-, 16-, 32- and 64-pixel tiles.
// A NaN pixel makes its tiles (-inf, +inf): no group over them is ever classified.
__global__ void __launch_bounds__(256) depth_tiles_kernel(const float* __restrict__ depth, int W, int H, float2* __restrict__ tiles, TileLevels tl) {
  __shared__ float2 s8[64], s16[16], s32[4];
  const int t = threadIdx.x;
  const int px = blockIdx.x * 64 + (t & 15) * 4, py = blockIdx.y * 64 + (t >> 4) * 4;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (py + j >= H) break;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (px + i >= W) break;
      const float d = depth[(size_t)(py + j) * W + px + i];
      if (d != d) { mn = -INFINITY; mx = INFINITY; }
      mn = fminf(mn, d); mx = fmaxf(mx, d);
    }
  }
  // 2 x 2 patches -> one 8-pixel tile: lanes (t & 15) ^ 1 and (t >> 4) ^ 1 (t ^ 1, t ^ 16)
  mn = fminf(mn, __shfl_xor(mn, 1)); mx = fmaxf(mx, __shfl_xor(mx, 1));
  mn = fminf(mn, __shfl_xor(mn, 16)); mx = fmaxf(mx, __shfl_xor(mx, 16));
  const int cx = (t & 15) >> 1, cy = t >> 5;          // 8 x 8 tiles of 8 pixels in this workgroup
  if (((t & 1) | ((t >> 4) & 1)) == 0) s8[cy * 8 + cx] = make_float2(mn, mx);
  __syncthreads();
  auto put = [&](int level, int lx, int ly, float2 v) {
    const int gx = blockIdx.x * (8 >> level) + lx, gy = blockIdx.y * (8 >> level) + ly;
    if (gx < tl.tw[level] && gy < tl.th[level]) tiles[tl.off[level] + gy * tl.tw[level] + gx] = v;
  };
  auto merge = [](float2 a, float2 b) { return make_float2(fminf(a.x, b.x), fmaxf(a.y, b.y)); };
  if (t < 64) put(0, t & 7, t >> 3, s8[t]);
  if (t < 16) {
    const int x = t & 3, y = t >> 2;
    const float2 v = merge(merge(s8[(2 * y) * 8 + 2 * x], s8[(2 * y) * 8 + 2 * x + 1]), merge(s8[(2 * y + 1) * 8 + 2 * x], s8[(2 * y + 1) * 8 + 2 * x + 1]));
    s16[t] = v; put(1, x, y, v);
  }
  __syncthreads();
  if (t < 4) {
    const int x = t & 1, y = t >> 1;
    const float2 v = merge(merge(s16[(2 * y) * 4 + 2 * x], s16[(2 * y) * 4 + 2 * x + 1]), merge(s16[(2 * y + 1) * 4 + 2 * x], s16[(2 * y + 1) * 4 + 2 * x + 1]));
    s32[t] = v; put(2, x, y, v);
  }
  __syncthreads();
  if (t == 0) put(3, 0, 0, merge(merge(s32[0], s32[1]), merge(s32[2], s32[3])));
}

// What the classification of a dense launch needs beside FuseParams.  A class covers the voxels x0 .. x0 + 3 of the rows y .. y + rows - 1
// (rows = 1: one group; rows = 4: a patch of the strip kernel).  Camera-space position of their centre, the voxel index
// (x0 + 1.5, y + (rows - 1) / 2, z): pc = C + x0 * Ax + y * Ay + z * Az (float, evaluated with FMAs: an approximation with a known error
// bound, never stored; make_group_classify puts the centre offset into C).  h*: half extent of those voxels in camera space,
// voxelSize * (1.5 |M column 0| + (rows - 1) / 2 |M column 1|).
struct GroupClassify {
  const float2* tiles;
  TileLevels tl;
  float Ax[3], Ay[3], Az[3], C[3];
  float hx, hy, hz;
  float slackZ;        // absolute slack on pc.z (metres): 1e-5 of the magnitudes that enter it
  int enabled;
};
enum { kGroupMixed = 0, kGroupFree = 1, kGroupShadow = 2 };

__device__ inline int classify_group(const GroupClassify& g, const FuseParams& p, int x0, int y, int z) {
  const float fx0 = (float)x0, fy = (float)y, fz = (float)z;
  const float pcx = __builtin_fmaf(g.Ax[0], fx0, __builtin_fmaf(g.Ay[0], fy, __builtin_fmaf(g.Az[0], fz, g.C[0])));
  const float pcy = __builtin_fmaf(g.Ax[1], fx0, __builtin_fmaf(g.Ay[1], fy, __builtin_fmaf(g.Az[1], fz, g.C[1])));
  const float pcz = __builtin_fmaf(g.Ax[2], fx0, __builtin_fmaf(g.Ay[2], fy, __builtin_fmaf(g.Az[2], fz, g.C[2])));
  const float ez = g.hz + g.slackZ;
  const float zmin = pcz - ez, zmax = pcz + ez;
  if (!(zmin > 1e-3f)) return kGroupMixed;                       // near or behind the camera plane (or NaN): exact path
  const float rz = __builtin_amdgcn_rcpf(pcz), rzmin = __builtin_amdgcn_rcpf(zmin) * 1.00001f;
  const float tx = pcx * rz, ty = pcy * rz;
  const float uc = __builtin_fmaf(p.fx, tx, p.cx), vc = __builtin_fmaf(p.fy, ty, p.cy);
  // |u(voxel) - u(centre)| <= fx (hx + |x / z| hz) / zmin exactly; + 0.5 for (int)(u + 0.5), + 1 pixel for the approximations here
  const float ru = fabsf(p.fx) * (g.hx + fabsf(tx) * g.hz) * rzmin + 1.5f + 1e-5f * fabsf(uc);
  const float rv = fabsf(p.fy) * (g.hy + fabsf(ty) * g.hz) * rzmin + 1.5f + 1e-5f * fabsf(vc);
  const float r = fmaxf(ru, rv);
  if (!(r <= 31.5f)) return kGroupMixed;
  const int level = (r <= 3.5f) ? 0 : (r <= 7.5f) ? 1 : (r <= 15.5f) ? 2 : 3;
  const float ulo = uc - ru, uhi = uc + ru, vlo = vc - rv, vhi = vc + rv;
  if (!(uhi >= 0.0f && vhi >= 0.0f && ulo <= (float)(p.W - 1) && vlo <= (float)(p.H - 1))) return kGroupMixed;   // footprint off the image: the column cull's business
  const bool inside = ulo >= 1.0f && vlo >= 1.0f && uhi <= (float)(p.W - 2) && vhi <= (float)(p.H - 2);
  const int sh = 3 + level;
  const int px0 = max((int)floorf(ulo), 0) >> sh, px1 = min((int)floorf(uhi), p.W - 1) >> sh;
  const int py0 = max((int)floorf(vlo), 0) >> sh, py1 = min((int)floorf(vhi), p.H - 1) >> sh;
  const float2* __restrict__ t = g.tiles + g.tl.off[level];
  const int tw = g.tl.tw[level];
  const float2 a = t[py0 * tw + px0], b = t[py0 * tw + px1], c = t[py1 * tw + px0], d = t[py1 * tw + px1];
  const float mn = fminf(fminf(a.x, b.x), fminf(c.x, d.x)), mx = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y));
  const float slack = 1e-5f * (fabsf(mx) + fabsf(mn) + zmax) + 1e-6f * p.mu;
  if (inside && (mn - zmax >= p.mu + slack)) return kGroupFree;        // every pixel valid (mn > 0 follows) and at least mu behind every voxel
  if (mx - zmin < -p.mu - slack) return kGroupShadow;                  // every pixel invalid or more than mu in front of every voxel
  return kGroupMixed;
}

// Dense volume of ITMVoxel_s with sx % 4 == 0: 4 voxels (16 B) per lane, one 1 KiB row segment per
// wave instruction; a group is written back only if one of its voxels changed.  blockIdx.y = z slice,
// blockIdx.x splits the (y, x/4) plane; no 64-bit index division in the loop, two 16-byte loads in
// flight per lane.
// Frustum planes of a dense launch in VOXEL-INDEX space, computed by the host in double:
//   g_k(xi, yi, zi) = a_k xi + b_k yi + cz_k zi + cm_k,   k = left, right, top, bottom, front
// with cm_k = c_k + margin_k, so that g_k < 0 for a voxel implies that the exact float test of fuse_depth_project rejects it
// (pc.z <= 0, or u / v outside [1, W-2] x [1, H-2]): margin_k = |a_k| + |b_k| (one voxel of slack along x and y) plus 1e-4 of
// the magnitudes that enter g_k, three orders above the rounding of the float evaluation.  nb_k = -1 / b_k (0 when b_k == 0).
struct ColumnCull {
  double a[5], nb[5], cz[5], cm[5];
  int kind[5];   // sign of b_k: +1 the plane bounds yi from below, -1 from above, 0 not at all (then g_k must be >= 0 as it is)
};

// Rows [rlo, rhi] of the column of groups (x0 .. x0 + 3, slice z) in which some voxel can pass the exact test (empty when rlo > rhi).
// Host and device: the same double-precision operations (fma is exactly rounded on both), so the host-side property test
// (tests/test_dense_cull.py, itm_debug_column_cull_rows) checks what the kernel computes.
__host__ __device__ inline void column_rows(const ColumnCull& cc, int x0, int z, int& rlo, int& rhi) {
  double ylo = -1e9, yhi = 1e9;
  bool none = false;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    // the largest value g_k takes on the group: at x0 + 3 when a_k > 0, at x0 otherwise
    const double t = __builtin_fma(cc.a[k], (double)(cc.a[k] > 0.0 ? x0 + 3 : x0), __builtin_fma(cc.cz[k], (double)z, cc.cm[k]));
    if (cc.kind[k] > 0) ylo = fmax(ylo, t * cc.nb[k]);          // b_k yi + t >= 0  <=>  yi >= -t / b_k
    else if (cc.kind[k] < 0) yhi = fmin(yhi, t * cc.nb[k]);     //                  <=>  yi <= -t / b_k   (b_k < 0)
    else none |= t < 0.0;
  }
  rlo = none ? 0x7fffffff : (int)ceil(fmax(ylo, -1e9));
  rhi = (int)floor(fmin(yhi, 1e9));
}

// ---- one 16-byte group of four ITMVoxel_s, as both kernels below treat it (each kernel stores the words itself) ------------------
// What the exact update saw of each voxel, for the check mode; every other caller ignores it and the compiler drops it.
struct GroupOutcome {
  float dm[4], eta[4];
  bool touched[4];
};

// The exact update of the voxels (xi .. xi + 3, my, mz), xi = x index + volume offset: project the four voxels, gather their depth
// pixels together (four independent loads in flight), then update.  True when a voxel changed.
__device__ inline bool group_exact(uint32_t v[4], int xi, float my, float mz, const float* __restrict__ depth, const FuseParams& p, GroupOutcome& o) {
  int pix[4]; float pcz[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    pix[k] = -1;
    if (p.stopAtMax && VoxelS::w_depth(v[k]) == p.maxW) continue;
    pix[k] = fuse_depth_project((float)(xi + k) * p.voxelSize, my, mz, p, pcz[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) o.dm[k] = (pix[k] >= 0) ? depth[pix[k]] : 0.0f;
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o.touched[k] = false;
    o.eta[k] = -1.0f;
    if (pix[k] >= 0) o.eta[k] = fuse_depth_update<VoxelS>(v[k], o.dm[k], pcz[k], p, o.touched[k]);
    any |= o.touched[k];
  }
  return any;
}

// Free-space group: the observation of every voxel is exactly 1 (fuse_depth_update with eta >= mu).  True when a voxel changed.
__device__ inline bool group_free(uint32_t v[4], const FuseParams& p) {
  bool any = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t w = (v[k] >> 16) & 0xffu;
    if (p.stopAtMax && (int)w == p.maxW) continue;
    uint32_t nv;
    if ((v[k] & 0xffffu) == 32767u) {            // (w * 1.0 + 1) / (w + 1) == 1.0 exactly: the sdf stays, the weight counts
      const int nw = ((int)w + 1 < p.maxW) ? (int)w + 1 : p.maxW;
      nv = 32767u | ((uint32_t)(nw & 0xff) << 16);
    } else {
      nv = v[k];
      fuse_average<VoxelS>(nv, 1.0f, p);
    }
    any |= nv != v[k];
    v[k] = nv;
  }
  return any;
}

// every weight at maxW: nothing of the group is integrated any more
__device__ inline bool group_saturated(const uint4& q, const FuseParams& p) {
  const uint32_t m = (uint32_t)(p.maxW & 0xff);
  return p.stopAtMax && ((q.x >> 16) & 0xffu) == m && ((q.y >> 16) & 0xffu) == m && ((q.z >> 16) & 0xffu) == m && ((q.w >> 16) & 0xffu) == m;
}

// CULL: 0 = per group with the exact arithmetic of two end voxels (any size); 1 = the rows [ylo, yhi] that can be inside the
// frustum are computed ONCE per thread for its column of groups (every group a thread visits has the same x0 when the stride
// is a multiple of the row length), the per-group test is then two integer comparisons.  Measured on BASELINE configs[2]
// (512^3): the per-group test was ~40 % of the kernel's VALU work (70 instructions for each of 33.5 M groups).
// CLASSIFY: 0 = every fetched group takes the exact per-voxel path; 1 = groups are classified against the depth tiles BEFORE they
// are fetched (shadow groups are never read); 2 = after the fetch, and only groups that still have an unsaturated voxel;
// 3 = measurement of the classification itself (itm_debug_dense_classify_check): classify, run the exact path, count disagreements.
__device__ int g_classifyCheck[4];     // CLASSIFY == 3: free groups, shadow groups, mixed groups, VIOLATIONS
template <bool POW2, int CULL, int CLASSIFY>
__global__ void __launch_bounds__(256) integrate_dense_s_x4_kernel(uint4* __restrict__ vba, const float* __restrict__ depth, FuseParams p,
                                                                   int sx, int sy, int sz, int ox, int oy, int oz, int log2sx4, ColumnCull cc, GroupClassify gc) {
  const int sx4 = sx >> 2;
  const int z = blockIdx.y;
  const int plane = sx4 * sy;                       // groups per z slice
  uint4* __restrict__ slice = vba + (size_t)z * plane;
  const float mz = (float)(z + oz) * p.voxelSize;
  const int stride = gridDim.x * 256;
  // idx -> (row, first voxel of the group)
  auto row_x0 = [&](int idx, int& y, int& x0) {
    y = POW2 ? (idx >> log2sx4) : (idx / sx4);
    x0 = (POW2 ? (idx & (sx4 - 1)) : (idx - y * sx4)) * 4;
  };
  auto group_class = [&](int idx) {
    int y, x0;
    row_x0(idx, y, x0);
    return classify_group(gc, p, x0, y, z);
  };
  auto process = [&](int idx, uint4 q, int cls) {
    if constexpr (CLASSIFY == 2) {
      if (group_saturated(q, p)) return;
      cls = group_class(idx);
    }
    uint32_t v[4] = {q.x, q.y, q.z, q.w};
    if constexpr (CLASSIFY == 1 || CLASSIFY == 2) {
      if (cls == kGroupShadow) return;
      if (cls == kGroupFree) {
        if (group_free(v, p)) slice[idx] = make_uint4(v[0], v[1], v[2], v[3]);
        return;
      }
    }
    int y, x0;
    row_x0(idx, y, x0);
    GroupOutcome o;
    const bool any = group_exact(v, x0 + ox, (float)(y + oy) * p.voxelSize, mz, depth, p, o);
    if constexpr (CLASSIFY == 3) {
      int bad = 0;
      uint32_t f[4] = {q.x, q.y, q.z, q.w};
      if (cls == kGroupFree) group_free(f, p);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool skipped = p.stopAtMax && VoxelS::w_depth((&q.x)[k]) == p.maxW;
        // free: every voxel that is not skipped must have been updated with an observation that clamps to 1
        if (cls == kGroupFree && !skipped && !(o.touched[k] && o.dm[k] > 0.0f && (p.muFast ? div_markstein(o.eta[k], p.mu, p.rcpMu) : o.eta[k] / p.mu) >= 1.0f)) ++bad;
        if (cls == kGroupShadow && o.touched[k]) ++bad;
        if (cls == kGroupFree && f[k] != v[k]) ++bad;        // and the shortcut -- the code that ships -- must produce the exact path's words
      }
      atomicAdd(&g_classifyCheck[cls == kGroupFree ? 0 : cls == kGroupShadow ? 1 : 2], 1);
      if (bad) atomicAdd(&g_classifyCheck[3], bad);
    }
    if (any) slice[idx] = make_uint4(v[0], v[1], v[2], v[3]);
  };
  // Conservative cull of a whole 4-voxel group BEFORE its 16 bytes are fetched: camera-space
  // coordinates are affine along x, so if both end voxels of the group lie outside the same frustum
  // plane (with half a pixel of margin, as in fuse_depth) every voxel of the group is rejected by the
  // exact per-voxel test as well.  ~70 % of a 512^3 volume around the camera is culled this way.
  auto culled = [&](int idx) {
    int y, x0;
    row_x0(idx, y, x0);
    const float my = (float)(y + oy) * p.voxelSize;
    const Vec3 a = transform_point(p.M_d, (float)(x0 + ox) * p.voxelSize, my, mz);
    const Vec3 b = transform_point(p.M_d, (float)(x0 + 3 + ox) * p.voxelSize, my, mz);
    const float lox = 0.5f - p.cx, hix = (float)(p.W - 2) + 0.5f - p.cx;
    const float loy = 0.5f - p.cy, hiy = (float)(p.H - 2) + 0.5f - p.cy;
    const float eps = 1e-3f * p.voxelSize;                 // margin on the z <= 0 plane
    const float atx = p.fx * a.x, aty = p.fy * a.y, btx = p.fx * b.x, bty = p.fy * b.y;
    // the four side planes are only meaningful for points in front of the camera
    const bool front = (a.z > eps) && (b.z > eps);
    return ((a.z < -eps) && (b.z < -eps)) ||
           (front && (((atx < lox * a.z) && (btx < lox * b.z)) || ((atx > hix * a.z) && (btx > hix * b.z)) ||
                      ((aty < loy * a.z) && (bty < loy * b.z)) || ((aty > hiy * a.z) && (bty > hiy * b.z))));
  };
  int idx = blockIdx.x * 256 + threadIdx.x;
  // rows of this thread's column (x0 .. x0 + 3, slice z) that may be inside the frustum
  [[maybe_unused]] int rlo = 0, rhi = 0;
  if constexpr (CULL == 1) column_rows(cc, (idx & (sx4 - 1)) * 4, z, rlo, rhi);
  // the class a group is processed with, or a negative value when it is not to be fetched: outside the column's rows, a shadow group
  // classified before the fetch (CLASSIFY == 3 reads everything: it checks the classes), culled by the per-group test
  auto want = [&](int i) {
    if constexpr (CULL == 1) {
      const int y = i >> log2sx4;
      if (y < rlo || y > rhi) return -1;
      if constexpr (CLASSIFY == 1 || CLASSIFY == 3) {
        const int k = group_class(i);
        return (CLASSIFY == 3 || k != kGroupShadow) ? k : -1;
      }
      return (int)kGroupMixed;
    } else {
      return culled(i) ? -1 : (int)kGroupMixed;
    }
  };
  // two groups per pass: both loads are issued before either group is processed
  for (; idx + stride < plane; idx += 2 * stride) {
    const int k0 = want(idx), k1 = want(idx + stride);
    uint4 q0, q1;
    if (k0 >= 0) q0 = slice[idx];
    if (k1 >= 0) q1 = slice[idx + stride];
    if (k0 >= 0) process(idx, q0, k0);
    if (k1 >= 0) process(idx + stride, q1, k1);
  }
  if (idx < plane) {
    const int k0 = want(idx);
    if (k0 >= 0) process(idx, slice[idx], k0);
  }
}

// ---- the strip kernel ------------------------------------------------------------------------------------------------------------
// What the counters say about the kernel above (profiles/r3_dense_counters.md, BASELINE configs[2]): 90 M vector instructions per
// launch, issue bound, and hardly fewer (81 M) once the weights have reached maxW -- the voxels in the SHADOW of the surface are
// never updated, so they never saturate and are projected in every frame, and a wave whose 64 lanes lie along x executes the
// projection for all of them as long as one lane needs it.  Classifying the groups against the depth tiles does not help that
// kernel (measured: 119 M instructions): its waves straddle the class boundaries, so nearly every wave still runs the exact path,
// now on top of the classification.
// Here the exact path is taken by PACKED lanes: a wave owns a strip (64 adjacent columns of 4-voxel groups of one z slice, 1 KiB of
// every row), takes four consecutive rows at a time -- a PATCH of 4 x 4 voxels per lane, classified once --, updates free-space patches
// in place, and QUEUES the groups of the patches that need the exact arithmetic in LDS; whenever 64 are waiting, they are taken off the queue and projected / gathered / averaged with every lane
// busy.  Shadow groups and saturated groups cost their classification only.  A strip is dealt out row by row over kStripPhases
// work items so that the waves working on it at one time read adjacent rows (waves each walking a row chunk 64 KB apart took
// 290 us for a 512^3 launch, whatever the arithmetic: all of them at the same offset modulo the chunk at the same time); items go
// round-robin over persistent waves, far slices first (a shared work counter was measured too: an atomic with a return value on
// one address is ~16 ns, serialised at the memory side -- 350 us for the 24 k draws of a launch).
constexpr int kStripPhases = 16;                 // work items per strip
constexpr int kStripQueue = 128;                 // queued groups per wave: fewer than 64 left over + at most 64 of one row

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) integrate_dense_strip_kernel(uint4* __restrict__ vba, const float* __restrict__ depth, FuseParams p,
                                                                    int sx, int sy, int sz, int ox, int oy, int oz, ColumnCull cc, GroupClassify gc) {
  __shared__ uint4 sQ[4][kStripQueue];
  __shared__ int sTag[4][kStripQueue];
  const int sx4 = sx >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int xblocks = (sx4 + 63) >> 6;
  const unsigned int perSlice = (unsigned int)(xblocks * kStripPhases);
  const unsigned int nItems = (unsigned int)sz * perSlice;
  const unsigned int nWaves = gridDim.x * (blockDim.x >> 6);
  for (unsigned int item = blockIdx.x * (blockDim.x >> 6) + wave; item < nItems; item += nWaves) {
    const int zi = (int)(item / perSlice), rem = (int)(item - (unsigned int)zi * perSlice);
    const int z = sz - 1 - zi;                                // far slices first
    const int phase = rem / xblocks, xb = rem - phase * xblocks;
    const int x4 = xb * 64 + lane, x0 = x4 * 4;
    uint4* __restrict__ slice = vba + (size_t)z * sx4 * sy;
    const float mz = (float)(z + oz) * p.voxelSize;
    int rlo, rhi;
    column_rows(cc, x0, z, rlo, rhi);
    rlo = max(rlo, 0); rhi = min(rhi, sy - 1);
    if (x4 >= sx4) { rlo = 1; rhi = 0; }                       // a row need not be a multiple of 64 groups
    // rows any lane of the wave needs (the loop bounds are the wave's, the test inside is the lane's)
    int wlo = (rlo <= rhi) ? rlo : 0x7fffffff, whi = (rlo <= rhi) ? rhi : -1;
#pragma unroll
    for (int off = 32; off; off >>= 1) { wlo = min(wlo, __shfl_xor(wlo, off)); whi = max(whi, __shfl_xor(whi, off)); }
    if (wlo > whi) continue;

    // the exact path for one queued group: tag = row * 64 + lane that queued it
    auto exact = [&](uint4 q, int tag) {
      const int y = tag >> 6, gx4 = xb * 64 + (tag & 63);
      uint32_t v[4] = {q.x, q.y, q.z, q.w};
      GroupOutcome o;
      if (group_exact(v, gx4 * 4 + ox, (float)(y + oy) * p.voxelSize, mz, depth, p, o)) slice[(size_t)y * sx4 + gx4] = make_uint4(v[0], v[1], v[2], v[3]);
    };
    int queued = 0;                                            // the same in every lane
    auto take = [&](int n) {                                   // the last n (<= 64) queued groups
      __builtin_amdgcn_wave_barrier();
      if (lane < n) exact(sQ[wave][queued - n + lane], sTag[wave][queued - n + lane]);
      __builtin_amdgcn_wave_barrier();
      queued -= n;
    };

    const uint4* __restrict__ dummy = slice + (size_t)wlo * sx4 + xb * 64;     // what a lane outside its interval reads (one line, dropped)
    // rows in PATCHES of four: patch G = rows 4 G .. 4 G + 3; this item takes the patches G = phase (mod kStripPhases)
    for (int G = (wlo >> 2) + (((phase - (wlo >> 2)) % kStripPhases + kStripPhases) % kStripPhases); 4 * G <= whi; G += kStripPhases) {
      const int y = 4 * G;
      uint4 qa[4];
      bool need[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = y + u >= rlo && y + u <= rhi;
        const uint4* a = in ? slice + (size_t)(y + u) * sx4 + x4 : dummy;
        qa[u] = *a;
        need[u] = in;
      }
      bool any = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool sat = group_saturated(qa[u], p);
        need[u] = need[u] && !sat;
        any |= need[u];
      }
      if (!__any(any)) continue;
      // one class for the 4 x 4 patch (gc was made for patches: centre (x0 + 1.5, y + 1.5), extents of both runs)
      const int cls = any ? classify_group(gc, p, x0, y, z) : kGroupShadow;
      if (cls == kGroupFree) {
        // every voxel of the patch observes free space: the observation is exactly 1 (fuse_depth_update with eta >= mu)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (!need[u]) continue;
          uint32_t v[4] = {qa[u].x, qa[u].y, qa[u].z, qa[u].w};
          if (group_free(v, p)) slice[(size_t)(y + u) * sx4 + x4] = make_uint4(v[0], v[1], v[2], v[3]);
        }
      }
      if (!__any(cls == kGroupMixed)) continue;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool mixed = cls == kGroupMixed && need[u];
        const unsigned long long m = __ballot(mixed);
        if (m) {
          if (mixed) {
            const int pos = queued + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            sQ[wave][pos] = qa[u]; sTag[wave][pos] = (y + u) * 64 + lane;
          }
          queued += __popcll(m);
          if (queued >= 64) take(64);
        }
      }
    }
    if (queued > 0) take(queued);
  }
}

// Camera space is affine in the voxel indices: pc_j = C[j] + xi Ax[j] + yi Ay[j] + zi Az[j] for the point (xi + cx, yi + cy, zi) of the
// index grid, from pc_j = M[j] mx + M[j+4] my + M[j+8] mz + M[j+12] with m = (index + offset) * voxelSize.  In double.
static void index_to_camera(const FuseParams& p, const int* off, double cx, double cy, double Ax[3], double Ay[3], double Az[3], double C[3]) {
  const double vs = p.voxelSize;
  for (int j = 0; j < 3; ++j) {
    const double m0 = p.M_d.m[j], m1 = p.M_d.m[j + 4], m2 = p.M_d.m[j + 8], m3 = p.M_d.m[j + 12];
    Ax[j] = m0 * vs; Ay[j] = m1 * vs; Az[j] = m2 * vs;
    C[j] = (m0 * (off[0] + cx) + m1 * (off[1] + cy) + m2 * off[2]) * vs + m3;
  }
}

// the classification's inputs for one launch; false when a coefficient is not finite (then nothing is classified)
// `rows`: 1 = a class per 4-voxel group; 4 = a class per PATCH of four such groups in consecutive rows (the strip kernel)
static bool make_group_classify(const FuseParams& p, const int* size, const int* off, const float2* tiles, const TileLevels& tl, GroupClassify& g, int rows = 1) {
  memset(&g, 0, sizeof g);
  g.tiles = tiles; g.tl = tl;
  const double vs = p.voxelSize;
  const double ry = 0.5 * (rows - 1);      // half extent along y in voxels
  double Ax[3], Ay[3], Az[3], C[3];
  index_to_camera(p, off, 1.5, ry, Ax, Ay, Az, C);       // centre of the run x0 .. x0 + 3 (of the rows y .. y + rows - 1)
  for (int j = 0; j < 3; ++j) {
    g.Ax[j] = (float)Ax[j]; g.Ay[j] = (float)Ay[j]; g.Az[j] = (float)Az[j]; g.C[j] = (float)C[j];
    if (!std::isfinite(g.Ax[j]) || !std::isfinite(g.Ay[j]) || !std::isfinite(g.Az[j]) || !std::isfinite(g.C[j])) return false;
  }
  const double mag = (fabs((double)p.M_d.m[2]) * (fabs((double)off[0]) + size[0]) + fabs((double)p.M_d.m[6]) * (fabs((double)off[1]) + size[1]) +
                      fabs((double)p.M_d.m[10]) * (fabs((double)off[2]) + size[2])) * vs + fabs((double)p.M_d.m[14]);
  g.hx = (float)((1.5 * fabs((double)p.M_d.m[0]) + ry * fabs((double)p.M_d.m[4])) * vs * 1.0001);
  g.hy = (float)((1.5 * fabs((double)p.M_d.m[1]) + ry * fabs((double)p.M_d.m[5])) * vs * 1.0001);
  g.hz = (float)((1.5 * fabs((double)p.M_d.m[2]) + ry * fabs((double)p.M_d.m[6])) * vs * 1.0001);
  g.slackZ = (float)(1e-5 * mag + 1e-7);
  g.enabled = 1;
  return std::isfinite(g.slackZ) && std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.cx) && std::isfinite(p.cy);
}

// The five frustum planes of ColumnCull from the launch parameters; false when a coefficient is not finite (then the per-group
// test runs).  pc_j = M[j] mx + M[j+4] my + M[j+8] mz + M[j+12] with m = (index + offset) * voxelSize is affine in the indices:
//   left   fx pc_x - (1 - cx) pc_z >= 0      right   ((W - 2) - cx) pc_z - fx pc_x >= 0
//   top    fy pc_y - (1 - cy) pc_z >= 0      bottom  ((H - 2) - cy) pc_z - fy pc_y >= 0      front  pc_z > 0
static bool make_column_cull(const FuseParams& p, const int* size, const int* off, ColumnCull& cc) {
  memset(&cc, 0, sizeof cc);
  const double vs = p.voxelSize;
  double Ax[3], Ay[3], Az[3], C[3];
  index_to_camera(p, off, 0.0, 0.0, Ax, Ay, Az, C);
  const double lox = 1.0 - (double)p.cx, hix = (double)(p.W - 2) - (double)p.cx, loy = 1.0 - (double)p.cy, hiy = (double)(p.H - 2) - (double)p.cy;
  const double fx = p.fx, fy = p.fy;
  // plane k as weights (wx, wy, wz) on (pc_x, pc_y, pc_z)
  const double w[5][3] = {{fx, 0, -lox}, {-fx, 0, hix}, {0, fy, -loy}, {0, -fy, hiy}, {0, 0, 1}};
  for (int k = 0; k < 5; ++k) {
    const double a = w[k][0] * Ax[0] + w[k][1] * Ax[1] + w[k][2] * Ax[2];
    const double b = w[k][0] * Ay[0] + w[k][1] * Ay[1] + w[k][2] * Ay[2];
    const double cz = w[k][0] * Az[0] + w[k][1] * Az[1] + w[k][2] * Az[2];
    const double c = w[k][0] * C[0] + w[k][1] * C[1] + w[k][2] * C[2];
    // magnitudes that enter g_k (not their sum, which may cancel)
    double mag = 0.0;
    for (int j = 0; j < 3; ++j)
      mag += fabs(w[k][j]) * (fabs(Ax[j]) * size[0] + fabs(Ay[j]) * size[1] + fabs(Az[j]) * size[2] +
                              (fabs((double)p.M_d.m[j] * off[0]) + fabs((double)p.M_d.m[j + 4] * off[1]) + fabs((double)p.M_d.m[j + 8] * off[2])) * vs + fabs((double)p.M_d.m[j + 12]));
    const double margin = fabs(a) + fabs(b) + 1e-4 * mag;
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(cz) || !std::isfinite(c) || !std::isfinite(margin)) return false;
    cc.a[k] = a; cc.cz[k] = cz; cc.cm[k] = c + margin;
    cc.kind[k] = (b > 0.0) ? 1 : (b < 0.0) ? -1 : 0;
    cc.nb[k] = (b != 0.0) ? -1.0 / b : 0.0;
    if (!std::isfinite(cc.nb[k])) { cc.kind[k] = 0; cc.nb[k] = 0.0; cc.cm[k] += fabs(b) * size[1]; }   // a slope too small to divide by: let the plane pass
  }
  return true;
}

// The six instantiations of the four-groups-per-lane kernel, by what the launch can use: without the column interval (a row that is no
// power of two groups, a stride that is no multiple of the row, debug key 9) the per-group cull and no classification, whatever key 16 says.
using DenseX4Kernel = void (*)(uint4*, const float*, FuseParams, int, int, int, int, int, int, int, ColumnCull, GroupClassify);
static DenseX4Kernel dense_x4_kernel(bool pow2, bool columns, int classify) {
  static const DenseX4Kernel byClass[4] = {integrate_dense_s_x4_kernel<true, 1, 0>, integrate_dense_s_x4_kernel<true, 1, 1>,
                                           integrate_dense_s_x4_kernel<true, 1, 2>, integrate_dense_s_x4_kernel<true, 1, 3>};
  if (columns) return byClass[classify];
  return pow2 ? integrate_dense_s_x4_kernel<true, 0, 0> : integrate_dense_s_x4_kernel<false, 0, 0>;
}

// The dense half of launch_integrate (integrate.hip), which has filled `p` and validated the view.
// (the integration timer brackets the integration kernel alone; the small depth-tile launch goes in front of it)
int launch_integrate_dense(itm_scene* s, const itm_view* v, const FuseParams& p, hipStream_t st) {
  const int* sz = s->cfg.denseSize; const int* of = s->cfg.denseOffset;
  if (s->cfg.voxelType != ITM_VOXEL_S || (sz[0] % 4) != 0) {
    KernelTimer tk(s, ITM_TK_INTEGRATE, st);
    return dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      integrate_dense_kernel<VX><<<256 * 32, 256, 0, st>>>(s->vba, v->depth, (const uchar4*)v->rgb, p, sz[0], sz[1], sz[2], of[0], of[1], of[2]);
      return ITM_OK;
    });
  }
  const int noStrips = debug_value(ITM_DEBUG_DENSE_NO_STRIPS), classifyMode = debug_value(ITM_DEBUG_DENSE_CLASSIFY);      // debug keys 17 and 16
  const int sx4 = sz[0] / 4;
  int lg = 0; while ((1 << lg) < sx4) ++lg;
  const bool pow2 = (1 << lg) == sx4;
  const int plane = sx4 * sz[1];
  int splits = (plane + 2 * 256 - 1) / (2 * 256);        // every lane gets ~2 groups per pass
  if (splits > 64) splits = 64;
  if (noStrips > 1) splits = noStrips;      // measurement: debug key 17 = n > 1 sets the number of splits of a slice
  if (splits < 1) splits = 1;
  ColumnCull cc;
  const bool planes = !debug_value(ITM_DEBUG_DENSE_GROUP_CULL) && make_column_cull(p, sz, of, cc);
  const bool columns = pow2 && ((splits * 256) % sx4) == 0 && planes;
  GroupClassify gc;
  memset(&gc, 0, sizeof gc);
  int classify = 0;
  const bool wantStrips = planes && !noStrips && classifyMode != 1 && classifyMode != 3 && sz[1] < (1 << 24);
  if (planes && classifyMode != 1) {
    // min / max depth tiles of this frame (one small launch), then groups are classified against them
    const TileLevels tl = tile_levels(v->w, v->h);
    if (s->depthTiles.reserve((size_t)tl.total) != hipSuccess) (void)hipGetLastError();
    if (s->depthTiles && make_group_classify(p, sz, of, s->depthTiles, tl, gc, wantStrips ? 4 : 1)) {
      depth_tiles_kernel<<<dim3((v->w + 63) / 64, (v->h + 63) / 64), 256, 0, st>>>(v->depth, v->w, v->h, s->depthTiles, tl);
      classify = classifyMode == 2 ? 2 : classifyMode == 3 ? 3 : 1;
    }
  }
  KernelTimer tk(s, ITM_TK_INTEGRATE, st);
  // the strip kernel: volumes whose rows are whole strips of 64 groups (debug key 17 keeps the launch shape of rounds 1-2)
  if (wantStrips && classify != 0) {
    // 16 384 waves for the 16 384 items of a 512^3 volume: one item each, dispatched as slots free up (measured, BASELINE configs[2]:
    // 1 024 workgroups 102-110 us, 2 048: 95-104, 3 072: 93-107, 4 096: 91-105)
    const int wgs = debug_value(ITM_DEBUG_INTEGRATE_WORKGROUPS) > 0 ? debug_value(ITM_DEBUG_INTEGRATE_WORKGROUPS) : 4096;
    integrate_dense_strip_kernel<<<wgs, 256, 0, st>>>((uint4*)s->vba.get(), v->depth, p, sz[0], sz[1], sz[2], of[0], of[1], of[2], cc, gc);
  } else {
    dense_x4_kernel(pow2, columns, classify)<<<dim3(splits, sz[2]), 256, 0, st>>>((uint4*)s->vba.get(), v->depth, p, sz[0], sz[1], sz[2], of[0], of[1], of[2], lg, cc, gc);
  }
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

// Test hook (host only, no device work): the row interval the dense integration would use for the column of 4-voxel groups
// (x0 .. x0 + 3, slice z) of a volume `size` / `offset` seen from pose M_d -- so that the conservativeness of the cull can be
// checked against the exact per-voxel test for thousands of poses on a machine without a GPU.  Returns 1 when the planes could not be formed.
extern "C" int itm_debug_column_cull_rows(const float M_d[16], const float intr[4], int w, int h, float voxelSize, const int size[3], const int offset[3],
                                          int x0, int z, int* rlo, int* rhi) {
  if (!M_d || !intr || !size || !offset || !rlo || !rhi) return set_error(ITM_ERR_INVALID, "null argument");
  FuseParams p;
  memset(&p, 0, sizeof p);
  memcpy(p.M_d.m, M_d, 64);
  p.fx = intr[0]; p.fy = intr[1]; p.cx = intr[2]; p.cy = intr[3];
  p.W = w; p.H = h; p.voxelSize = voxelSize;
  ColumnCull cc;
  if (!make_column_cull(p, size, offset, cc)) return 1;
  column_rows(cc, x0, z, *rlo, *rhi);
  return ITM_OK;
}

// Test hook: the counters of the classification check (debug key 16 = 3): {free groups, shadow groups, mixed groups, violations};
// reset != 0 clears them.  A violation is a voxel of a classified group whose exact per-voxel outcome differs from its class.
extern "C" int itm_debug_dense_classify_check(int32_t out[4], int reset) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  ITM_HIP(hipDeviceSynchronize());
  ITM_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_classifyCheck), 16));
  if (reset) { const int32_t z[4] = {0, 0, 0, 0}; ITM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_classifyCheck), z, 16)); }
  return ITM_OK;
}
