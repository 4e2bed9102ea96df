// query.hip -- the scene asked at caller-supplied points and along caller-supplied rays (include/itm_hip.h: itm_scene_query_points,
// itm_scene_cast_rays): the reads the engines make per pixel, with a work item that is not a pixel.
//
// Reference behaviour restated (every value through the functions the renders and the mesh attributes already use):
//   readFromSDF_float_uninterpolated / _interpolated  DeviceAgnostic/ITMRepresentationAccess.h:144-185   (volume_device.h)
//   readFromSDF_color4u_interpolated                  :187-222                                           (sample_device.h: colour_from)
//   computeSingleNormalFromSDF                        :224-337                                           (sample_device.h: gradient_axis)
//   readVoxel: an absent voxel reads TVoxel()         :85-142
//   castRay                                           DeviceAgnostic/ITMVisualisationEngine.h:92-158     (raycast_device.h: march_segment)
//
// MI355X design.  One lane per point (or ray), 256-lane workgroups, grid-stride; no LDS: the points are unrelated, what neighbouring
// lanes share they share through L2.  The point kernel is compiled per KIND OF READ the wanted outputs need (kTri / kGrad / kColour;
// the single voxel of `weight` / a lone `sdf_nearest` is a wave-uniform branch): a caller that wants only `sdf` pays the eight loads of
// Corners::fetch.  The gradient reads floor(p) + [-1, 2]^3 minus the cells with two coordinates outside {0, 1}: 32 voxels that CONTAIN
// the eight corners of the trilinear cell, so with kGrad one gather serves sdf, sdf_nearest, gradient, normal and the flags.  The
// gather (fetch_gradient_taps) follows Corners::fetch: the 4-voxel span crosses at most one block face per axis, so at most eight
// blocks are involved -- their bases are resolved together (dense sdf mirror: none needed, the address follows from the position;
// paged mirror: eight page-table reads; block directory: eight cells; table walk: eight head entries, then the chains), then all 32
// loads are issued back to back from addresses that are always valid, and only then is the first value used.  The colours' eight
// full-voxel loads go through the same resolved blocks.  A lane whose point is invalid samples position (0, 0, 0) and drops the values.
#include "itm_internal.h"
#include "raycast_device.h"
#include "sample_device.h"

namespace itm {

enum : uint32_t { kTri = 1u, kGrad = 2u, kColour = 4u };

struct QueryOut { float* sdf; float* nearest; float* gradient; float* normal; uchar4* colour; uint8_t* weight; uint32_t* flags; };

constexpr float kPointLimit = 262136.0f;     // floor(p) - 1 .. floor(p) + 2 stay inside the table's short block coordinates
constexpr float kRayLimit = 131072.0f;       // end points of a ray, voxels
constexpr float kRayLengthLimit = 4194304.0f;   // |t| in voxels: below 2^24, where `total += step` still moves for every step >= 1

__device__ inline int pick8(const int b[8], bool tx, bool ty, bool tz) {      // b[tx | ty << 1 | tz << 2] as a tree of selects
  const int x0 = tx ? b[1] : b[0], x1 = tx ? b[3] : b[2], x2 = tx ? b[5] : b[4], x3 = tx ? b[7] : b[6];
  const int y0 = ty ? x1 : x0, y1 = ty ? x3 : x2;
  return tz ? y1 : y0;
}

// The up-to-eight blocks a span of voxels [lo, lo + SPAN) per axis (SPAN <= 8) touches: base[s] = first voxel of the block at
// (bx + (s & 1), by + ((s >> 1) & 1), bz + (s >> 2)) for the s with (s & ~cross) == 0 -- cross bit k: the span reaches the next block
// along axis k -- and base[s & cross] for the others; -1 where no block is allocated.  Corners::fetch's general path for any span,
// without its "the lane is still in its cached block" short cut: a point's BlockCache is fresh when this runs, once per point.  The
// first block is left in the cache for the single-voxel read of `weight` that may follow.
__device__ inline void resolve_blocks(const VolumeView& vol, int bx, int by, int bz, int cross, BlockCache& cache, int base[8]) {
  const uint32_t ux = (uint32_t)(bx - vol.org.dx), uy = (uint32_t)(by - vol.org.dy), uz = (uint32_t)(bz - vol.org.dz);
  const bool viaDir = vol.dirPtr && dir_covers(ux, uy, uz) && dir_covers(ux + 1u, uy + 1u, uz + 1u);
  if (__any(viaDir)) {
    int ptr[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int t = s & cross;
      const uint32_t cell = viaDir ? dir_cell(ux + (uint32_t)(t & 1), uy + (uint32_t)((t >> 1) & 1), uz + (uint32_t)(t >> 2)) : 0u;
      ptr[s] = vol.dirPtr[cell];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) base[s] = (ptr[s] < 0) ? -1 : ptr[s] * kBlockVoxels;
  }
  if (!viaDir) {
    // outside the directory (or directory disabled): table walk; entries are fetched for the blocks actually needed, the other loads
    // re-read the first entry
    const int idx0 = hash_index(bx, by, bz, vol.mask);
    HashEntry head[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool need = (s & ~cross) == 0;
      head[s] = unpack_entry(vol.hash[need ? hash_index(bx + (s & 1), by + ((s >> 1) & 1), bz + (s >> 2), vol.mask) : idx0]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool need = (s & ~cross) == 0;
      base[s] = need ? resolve_block(vol, head[s], bx + (s & 1), by + ((s >> 1) & 1), bz + (s >> 2)) : -1;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) base[s] = base[s & cross];
  }
  if (base[0] >= 0) { cache.bx = bx; cache.by = by; cache.bz = bz; cache.base = base[0]; }
}

// a voxel span per axis: first voxel `lo`, its block, whether the span's last voxel lies in the next block
struct Span {
  int lx, ly, lz, bx, by, bz, cross;
  __device__ Span(int x, int y, int z, int last) : lx(x), ly(y), lz(z), bx(x >> 3), by(y >> 3), bz(z >> 3) {
    cross = (((x + last) >> 3) != bx ? 1 : 0) | (((y + last) >> 3) != by ? 2 : 0) | (((z + last) >> 3) != bz ? 4 : 0);
  }
  // voxel index of the span's voxel (ax, ay, az) (offsets from lo) through the resolved blocks; -1 where no block is allocated
  __device__ int locate(const int base[8], int ax, int ay, int az) const {
    const int x = lx + ax, y = ly + ay, z = lz + az;
    const int b = pick8(base, (x >> 3) != bx, (y >> 3) != by, (z >> 3) != bz);
    return b < 0 ? -1 : b + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6);
  }
};

constexpr bool grad_tap(int a, int b, int c) {      // offsets 0 .. 3 (= -1 .. 2): at least two coordinates inside the cell
  return ((a == 1 || a == 2) ? 1 : 0) + ((b == 1 || b == 2) ? 1 : 0) + ((c == 1 || c == 2) ? 1 : 0) >= 2;
}

// The 32 voxels computeSingleNormalFromSDF reads around floor(p) = (ix, iy, iz): raw sdf in v[dz + 1][dy + 1][dx + 1] (the default
// voxel's where none is stored) and whether a voxel is stored there.  `base`: the span's blocks when `resolved` (the caller needs
// them for the colours), else resolved here if the mirror does not serve the wave.
template <class VX, bool DENSE>
__device__ inline void fetch_gradient_taps(const VolumeView& vol, int ix, int iy, int iz, BlockCache& cache, int base[8], bool resolved,
                                           float v[4][4][4], bool present[4][4][4]) {
  const float dflt = VX::kShort ? 32767.0f : 1.0f;
  const int x0 = ix - 1, y0 = iy - 1, z0 = iz - 1;
  if constexpr (DENSE) {
    uint32_t at[4][4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) at[c][b][a] = dense_lin(vol, x0 + a, y0 + b, z0 + c, present[c][b][a]);
    float raw[4][4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) raw[c][b][a] = VX::load_raw_sdf(vol.vba, (size_t)at[c][b][a]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) v[c][b][a] = present[c][b][a] ? raw[c][b][a] : dflt;
    return;
  } else {
    using MC = MirrorCodec<VX::kShort>;
    using MT = typename MC::T;
    const MT* mirror = (const MT*)vol.sdfMirror;
    bool served = false;      // (wave-uniform)
    if (mirror && mirror_is_dense(vol)) {
      // DENSE cube: the address follows from the position.  Taken when the block of the span's first voxel and the next one per axis
      // lie in the cube (one more than the span may need at the upper faces, where the general path gives the same values)
      const uint32_t mx = (uint32_t)((x0 >> 3) - vol.org.mx), my = (uint32_t)((y0 >> 3) - vol.org.my), mz = (uint32_t)((z0 >> 3) - vol.org.mz);
      const int mbits = mirror_dense_bits(vol.org);
      const bool all = mirror_dense_covers(mx, my, mz, mbits) && mirror_dense_covers(mx + 1u, my + 1u, mz + 1u, mbits);
      if (__all(all)) {
        MT m[4][4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a)
              if (grad_tap(a, b, c)) {
                const int x = x0 + a, y = y0 + b, z = z0 + c;
                const uint32_t cell = mirror_dense_cell((uint32_t)((x >> 3) - vol.org.mx), (uint32_t)((y >> 3) - vol.org.my), (uint32_t)((z >> 3) - vol.org.mz), mbits);
                m[c][b][a] = mirror[((size_t)cell << 9) | (size_t)((x & 7) + ((y & 7) << 3) + ((z & 7) << 6))];
              }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a)
              if (grad_tap(a, b, c)) { present[c][b][a] = !MC::absent(m[c][b][a]); v[c][b][a] = present[c][b][a] ? MC::raw(m[c][b][a]) : dflt; }
        served = true;
      }
    } else if (mirror && mirror_is_paged(vol)) {
      // PAGED cube: the span touches at most two pages per axis -- the eight candidates' table entries, then the 32 values
      const uint32_t vx = (uint32_t)(x0 - (vol.org.mx << 3)), vy = (uint32_t)(y0 - (vol.org.my << 3)), vz = (uint32_t)(z0 - (vol.org.mz << 3));
      const bool inCube = mirror_covers_voxel(vx, vy, vz) && mirror_covers_voxel(vx + 3u, vy + 3u, vz + 3u);
      if (__all(inCube)) {
        int pg[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) pg[s] = vol.pageTable[mirror_table_index_voxel(vx + ((s & 1) ? 3u : 0u), vy + ((s & 2) ? 3u : 0u), vz + ((s & 4) ? 3u : 0u))];
        bool usable = true;
#pragma unroll
        for (int s = 0; s < 8; ++s) usable &= pg[s] != kPageUnmappable;
        if (__all(usable)) {
          MT got[4][4][4];
          int page[4][4][4];
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
              for (int a = 0; a < 4; ++a)
                if (grad_tap(a, b, c)) {
                  const uint32_t qx = vx + (uint32_t)a, qy = vy + (uint32_t)b, qz = vz + (uint32_t)c;
                  const int p = pick8(pg, (qx >> kPageVoxBits) != (vx >> kPageVoxBits), (qy >> kPageVoxBits) != (vy >> kPageVoxBits), (qz >> kPageVoxBits) != (vz >> kPageVoxBits));
                  page[c][b][a] = p;
                  got[c][b][a] = mirror[p >= 0 ? mirror_element(p, mirror_in_page(qx, qy, qz)) : (size_t)0];
                }
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
              for (int a = 0; a < 4; ++a)
                if (grad_tap(a, b, c)) {
                  const MT mv = page[c][b][a] >= 0 ? got[c][b][a] : MC::kAbsent;
                  present[c][b][a] = !MC::absent(mv); v[c][b][a] = present[c][b][a] ? MC::raw(mv) : dflt;
                }
          served = true;
        }
      }
    }
    if (served) return;
    // block directory / table walk: the span's blocks, then the 32 voxels
    const Span sp(x0, y0, z0, 3);
    if (!resolved) resolve_blocks(vol, sp.bx, sp.by, sp.bz, sp.cross, cache, base);
    int at[4][4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) at[c][b][a] = sp.locate(base, a, b, c);
    float raw[4][4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) raw[c][b][a] = VX::load_raw_sdf(vol.vba, at[c][b][a] < 0 ? (size_t)0 : (size_t)at[c][b][a]);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a)
          if (grad_tap(a, b, c)) { present[c][b][a] = at[c][b][a] >= 0; v[c][b][a] = present[c][b][a] ? raw[c][b][a] : dflt; }
  }
}

template <class VX, bool DENSE, uint32_t WORK>
__global__ void __launch_bounds__(256) query_points_kernel(VolumeView vol, const float* __restrict__ points, uint32_t n, float voxelSize, bool metres, QueryOut out) {
  constexpr bool TRI = (WORK & kTri) != 0, GRAD = (WORK & kGrad) != 0, COLOUR = (WORK & kColour) != 0 && VX::kColor;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    const float* q = points + 3 * i;
    float px = q[0], py = q[1], pz = q[2];
    if (metres) { px = px / voxelSize; py = py / voxelSize; pz = pz / voxelSize; }
    const bool valid = (fabsf(px) < kPointLimit) && (fabsf(py) < kPointLimit) && (fabsf(pz) < kPointLimit);      // false for NaN and Inf too
    if (!valid) px = py = pz = 0.0f;
    BlockCache cache;
    Corners<VX, DENSE> cn;
    float g[3] = {0.0f, 0.0f, 0.0f};
    uchar4 clr = make_uchar4(0, 0, 0, 0);
    int base[8];
    const float flx = floorf(px), fly = floorf(py), flz = floorf(pz);
    const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
    // the blocks the colours (and, without a mirror, the gradient's voxels) are read through: resolved once for the wider span
    const Span sp = GRAD ? Span(ix - 1, iy - 1, iz - 1, 3) : Span(ix, iy, iz, 1);
    if constexpr (COLOUR && !DENSE) resolve_blocks(vol, sp.bx, sp.by, sp.bz, sp.cross, cache, base);
    if constexpr (GRAD) {
      float v[4][4][4];
      bool present[4][4][4];
      fetch_gradient_taps<VX, DENSE>(vol, ix, iy, iz, cache, base, COLOUR && !DENSE, v, present);
      cn.cx = px - flx; cn.cy = py - fly; cn.cz = pz - flz;
      cn.ix = ix; cn.iy = iy; cn.iz = iz;
#pragma unroll
      for (int c = 0; c < 8; ++c) { cn.v[c] = v[1 + (c >> 2)][1 + ((c >> 1) & 1)][1 + (c & 1)]; cn.present[c] = present[1 + (c >> 2)][1 + ((c >> 1) & 1)][1 + (c & 1)]; }
      auto raw = [&](int dx, int dy, int dz) { return v[dz + 1][dy + 1][dx + 1]; };
      g[0] = gradient_axis<VX, 0>(raw, cn.cx, cn.cy, cn.cz);
      g[1] = gradient_axis<VX, 1>(raw, cn.cy, cn.cx, cn.cz);
      g[2] = gradient_axis<VX, 2>(raw, cn.cz, cn.cx, cn.cy);
    } else if constexpr (TRI) {
      cn.fetch(vol, px, py, pz, cache);
    }
    if constexpr (COLOUR) {
      const int o = GRAD ? 1 : 0;      // the cell's first voxel inside the span
      typename VX::Reg reg[8];
      bool has[8];
      if constexpr (DENSE) {
        uint32_t at[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) at[c] = dense_lin(vol, ix + (c & 1), iy + ((c >> 1) & 1), iz + (c >> 2), has[c]);
#pragma unroll
        for (int c = 0; c < 8; ++c) reg[c] = VX::load(vol.vba, (size_t)at[c]);
      } else {
        int at[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) at[c] = sp.locate(base, o + (c & 1), o + ((c >> 1) & 1), o + (c >> 2));
#pragma unroll
        for (int c = 0; c < 8; ++c) { has[c] = at[c] >= 0; reg[c] = VX::load(vol.vba, has[c] ? (size_t)at[c] : (size_t)0); }
      }
      uint32_t packed8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        int rgb[3], wc;
        VX::get_color(reg[c], rgb, wc);
        packed8[c] = has[c] ? ((uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16)) : 0u;
      }
      auto packed = [&](int dx, int dy, int dz) { return packed8[dx + 2 * dy + 4 * dz]; };
      clr = colour_bytes(colour_from(packed, px - flx, py - fly, pz - flz));
    }
    // the voxel at ROUND(p)
    bool found = false;
    float nearest = 1.0f;
    if constexpr (TRI || GRAD) nearest = cn.nearest(px, py, pz, found);
    else if (out.nearest) nearest = sdf_nearest<VX, DENSE>(vol, px, py, pz, found, cache);      // (uniform)
    int weight = 0;
    if (out.weight) {      // (uniform) the stored voxel itself: the mirror holds the sdf alone
      const long long a = locate_voxel<DENSE>(vol, (int)round_ref(px), (int)round_ref(py), (int)round_ref(pz), cache);
      const typename VX::Reg r = VX::load(vol.vba, a < 0 ? (size_t)0 : (size_t)a);
      weight = a < 0 ? 0 : VX::w_depth(r);
    }
    if constexpr (TRI || GRAD) {
      if (out.sdf) out.sdf[i] = valid ? cn.trilinear() : 1.0f;
    }
    if (out.nearest) out.nearest[i] = valid ? nearest : 1.0f;
    if (out.gradient) { float* o = out.gradient + 3 * i; o[0] = valid ? g[0] : 0.0f; o[1] = valid ? g[1] : 0.0f; o[2] = valid ? g[2] : 0.0f; }
    if (out.normal) {
      if (valid) store_normal(out.normal + 3 * i, g[0], g[1], g[2]);
      else { float* o = out.normal + 3 * i; o[0] = o[1] = o[2] = 0.0f; }
    }
    if (out.colour) out.colour[i] = valid ? clr : make_uchar4(0, 0, 0, 0);
    if (out.weight) out.weight[i] = valid ? (uint8_t)weight : (uint8_t)0;
    if constexpr (TRI || GRAD) if (out.flags) {
      uint32_t f = found ? 1u : 0u, corners = 0u;
#pragma unroll
      for (int c = 0; c < 8; ++c) corners |= cn.present[c] ? (1u << c) : 0u;
      f |= (corners << 8) | (corners == 0xffu ? 2u : 0u);
      out.flags[i] = valid ? f : (uint32_t)ITM_QUERY_INVALID;
    }
  }
}

template <class VX, bool DENSE>
__global__ void __launch_bounds__(256) cast_rays_kernel(VolumeView vol, const float* __restrict__ rays, uint32_t n, float oneOverVoxel, float stepScale, float4* __restrict__ hits) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
    const float* q = rays + 8 * i;
    const float sx = q[0] * oneOverVoxel, sy = q[1] * oneOverVoxel, sz = q[2] * oneOverVoxel, t0 = q[3] * oneOverVoxel;
    const float ex = q[4] * oneOverVoxel, ey = q[5] * oneOverVoxel, ez = q[6] * oneOverVoxel, t1 = q[7] * oneOverVoxel;
    RaySetup r;
    float dx = ex - sx, dy = ey - sy, dz = ez - sz;
    const float dn = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
    r.dx = dx * dn; r.dy = dy * dn; r.dz = dz * dn;
    r.px = sx; r.py = sy; r.pz = sz; r.total = t0; r.totalMax = t1;
    // (the comparisons are false for NaN and Inf; scaled values of finite input that overflowed are refused with them)
    const bool valid = (fabsf(sx) < kRayLimit) && (fabsf(sy) < kRayLimit) && (fabsf(sz) < kRayLimit) && (fabsf(ex) < kRayLimit) && (fabsf(ey) < kRayLimit) &&
                       (fabsf(ez) < kRayLimit) && (fabsf(t0) < kRayLengthLimit) && (fabsf(t1) < kRayLengthLimit) && !(sx == ex && sy == ey && sz == ez) &&
                       __builtin_isfinite(r.dx) && __builtin_isfinite(r.dy) && __builtin_isfinite(r.dz);
    if (!valid) { r.px = r.py = r.pz = r.dx = r.dy = r.dz = 0.0f; r.total = r.totalMax = 0.0f; }      // no step: total < totalMax is false
    const float4 h = march_segment<VX, DENSE>(r, stepScale, vol);
    hits[i] = valid ? h : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

template <class VX, bool DENSE>
static void launch_points(uint32_t work, int grid, hipStream_t st, const VolumeView& vol, const float* pts, uint32_t n, float voxelSize, bool metres, const QueryOut& o) {
#define ITM_Q(W) case W: query_points_kernel<VX, DENSE, W><<<grid, 256, 0, st>>>(vol, pts, n, voxelSize, metres, o); break;
  if constexpr (VX::kColor) {
    switch (work) { ITM_Q(0u) ITM_Q(kTri) ITM_Q(kTri | kGrad) ITM_Q(kColour) ITM_Q(kTri | kColour) ITM_Q(kTri | kGrad | kColour) }
  } else {
    switch (work) { ITM_Q(0u) ITM_Q(kTri) ITM_Q(kTri | kGrad) }
  }
#undef ITM_Q
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_scene_query_points(const itm_scene* s, const float* points_dev, uint32_t n, int units, const itm_query_out* out, itm_stream stream) {
  if (!s || !out) return set_error(ITM_ERR_INVALID, "null argument");
  if (units != ITM_QUERY_METRES && units != ITM_QUERY_VOXELS) return set_error(ITM_ERR_INVALID, "units: ITM_QUERY_METRES or ITM_QUERY_VOXELS");
  if (out->colour && !voxel_has_colour(s->cfg.voxelType))
    return set_error(ITM_ERR_INVALID, "the scene's voxel type stores no colour: a query has no colour output");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  if (n == 0) return ITM_OK;
  if (!points_dev) return set_error(ITM_ERR_INVALID, "null points");
  QueryOut o = {out->sdf, out->sdf_nearest, out->gradient, out->normal, (uchar4*)out->colour, out->weight, out->flags};
  if (!(o.sdf || o.nearest || o.gradient || o.normal || o.colour || o.weight || o.flags)) return ITM_OK;      // nothing wanted
  uint32_t work = 0;
  if (o.gradient || o.normal) work |= kGrad | kTri;      // the gradient's voxels contain the cell's corners
  if (o.sdf || o.flags) work |= kTri;
  if (o.colour) work |= kColour;
  hipStream_t st = as_stream(stream);
  const VolumeView vol = make_volume(s);
  const uint32_t groups = (n + 255u) / 256u;
  const int grid = (int)(groups < 2048u ? groups : 2048u);
  const int rc = dispatch_volume(s, [&](auto vx, auto dense) {
    launch_points<decltype(vx), dense.value>(work, grid, st, vol, points_dev, n, s->prm.voxelSize, units == ITM_QUERY_METRES, o);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

int itm_scene_cast_rays(const itm_scene* s, const float* rays_dev, uint32_t n, float* hits_dev, itm_stream stream) {
  if (!s) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  if (n == 0) return ITM_OK;
  if (!rays_dev || !hits_dev) return set_error(ITM_ERR_INVALID, "null argument");
  if (((uintptr_t)hits_dev & 15u) != 0) return set_error(ITM_ERR_INVALID, "hits_dev must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const VolumeView vol = make_volume(s);
  const float oneOverVoxel = 1.0f / s->prm.voxelSize, stepScale = s->prm.mu * oneOverVoxel;      // as make_ray_params / march_ray form them
  const uint32_t groups = (n + 255u) / 256u;
  const int grid = (int)(groups < 2048u ? groups : 2048u);
  const int rc = dispatch_volume(s, [&](auto vx, auto dense) {
    cast_rays_kernel<decltype(vx), dense.value><<<grid, 256, 0, st>>>(vol, rays_dev, n, oneOverVoxel, stepScale, (float4*)hits_dev);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // extern "C"
