// colour_tracker.hip -- photometric (colour) tracker: aligns the rgb image of a view with the coloured point cloud of the
// scene that CreatePointCloud wrote (visualise_aux.hip).
//
// Reference behaviour:
//   filterSubsample (uchar4), gradientX / gradientY   DeviceAgnostic/ITMLowLevelEngine.h:7-24,73-123 (CPU loops: _CPU.cpp:35-104)
//   getColorDifferenceSq, computePerPointGH_rt_Color  DeviceAgnostic/ITMColorTracker.h
//   interpolateBilinear                               DeviceAgnostic/ITMPixelUtils.h:11-39
//   ITMColorTracker_CPU::F_oneLevel / G_oneLevel      DeviceSpecific/CPU/ITMColorTracker_CPU.cpp:14-101
//   ITMColorTracker::TrackCamera / minimizeLM         Engine/ITMColorTracker.cpp (host loop: colour_solver.h)
//
// Device part: two launches prepare the pyramid (all coarser levels from one pass over the input, then both gradients of every
// level); one launch per evaluation, one lane per point, computes the squared colour difference and -- in the same pass -- the
// gradient / Hessian terms with the reference's float operations (projection with IEEE division, no contraction: the valid count
// is exact), and reduces them with the ICP tracker's fixed-order double tree (gh_reduce.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

#include "itm_internal.h"
#include "gh_reduce.h"
#include "colour_solver.h"
#include "se3.h"

namespace itm {

constexpr int kColourMaxLevels = 8;

struct ColourPyramid {
  uchar4* rgb[kColourMaxLevels];
  short4* gx[kColourMaxLevels];
  short4* gy[kColourMaxLevels];
  int w[kColourMaxLevels], h[kColourMaxLevels];
  int levels;
};

// Up to four FilterSubsample levels below `first` in one launch: a level-(first+l) pixel depends on a 2^l x 2^l block of level
// `first` only, so a workgroup that owns a 16x16 tile of it produces every coarser pixel under it through LDS (the same nested
// truncating averages as one launch per level).  Workgroups of the first launch also copy level 0 from the view.
__global__ void __launch_bounds__(256) colour_pyramid_kernel(const uchar4* __restrict__ in, ColourPyramid P, int first, int count,
                                                             uchar4* __restrict__ copy) {
  __shared__ uchar4 tile[2][16][16];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int gx = blockIdx.x * 16 + tx, gy = blockIdx.y * 16 + ty;
  const int W = P.w[first], H = P.h[first];
  uchar4 v = make_uchar4(0, 0, 0, 0);
  if (gx < W && gy < H) {
    v = in[gx + gy * W];
    if (copy) copy[gx + gy * W] = v;
  }
  tile[0][ty][tx] = v;                    // pixels outside the level are never read by a pixel of a coarser level (floor halves)
  __syncthreads();
  int side = 8, cur = 0;
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    if (l < count) {
      if (tx < side && ty < side) {
        const uchar4 a = tile[cur][2 * ty][2 * tx], b = tile[cur][2 * ty][2 * tx + 1], c = tile[cur][2 * ty + 1][2 * tx],
                     d = tile[cur][2 * ty + 1][2 * tx + 1];
        uchar4 o;
        o.x = (unsigned char)(((int)a.x + (int)b.x + (int)c.x + (int)d.x) / 4);
        o.y = (unsigned char)(((int)a.y + (int)b.y + (int)c.y + (int)d.y) / 4);
        o.z = (unsigned char)(((int)a.z + (int)b.z + (int)c.z + (int)d.z) / 4);
        o.w = (unsigned char)(((int)a.w + (int)b.w + (int)c.w + (int)d.w) / 4);
        tile[cur ^ 1][ty][tx] = o;
        const int lv = first + 1 + l, ox = blockIdx.x * side + tx, oy = blockIdx.y * side + ty;
        if (ox < P.w[lv] && oy < P.h[lv]) P.rgb[lv][ox + oy * P.w[lv]] = o;
      }
      __syncthreads();
      cur ^= 1; side >>= 1;
    }
  }
}

// gradientX and gradientY of every level in one launch: blockIdx.y = level.  Interior pixels as the reference (int differences,
// truncating division by 8, .w = (510 + 1020 + 510) / 8 = 255); border rows and columns 0 (never written by the reference, whose
// buffers start zeroed).
__global__ void __launch_bounds__(256) colour_gradient_kernel(ColourPyramid P) {
  const int lv = blockIdx.y;
  const int W = P.w[lv], H = P.h[lv];
  const uchar4* __restrict__ im = P.rgb[lv];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < W * H; i += gridDim.x * 256) {
    const int x = i % W, y = i / W;
    short4 gx = make_short4(0, 0, 0, 0), gy = make_short4(0, 0, 0, 0);
    if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
      const uchar4 nw = im[i - W - 1], n = im[i - W], ne = im[i - W + 1];
      const uchar4 w = im[i - 1], e = im[i + 1];
      const uchar4 sw = im[i + W - 1], s = im[i + W], se = im[i + W + 1];
      // d = (d1 + 2 d2 + d3) / 8: differences of at most 255 in magnitude, int arithmetic, division truncating toward zero
      auto tap = [](int d1, int d2, int d3) { return (d1 + 2 * d2 + d3) / 8; };
      gx.x = (short)tap((int)ne.x - (int)nw.x, (int)e.x - (int)w.x, (int)se.x - (int)sw.x);
      gx.y = (short)tap((int)ne.y - (int)nw.y, (int)e.y - (int)w.y, (int)se.y - (int)sw.y);
      gx.z = (short)tap((int)ne.z - (int)nw.z, (int)e.z - (int)w.z, (int)se.z - (int)sw.z);
      gy.x = (short)tap((int)sw.x - (int)nw.x, (int)s.x - (int)n.x, (int)se.x - (int)ne.x);
      gy.y = (short)tap((int)sw.y - (int)nw.y, (int)s.y - (int)n.y, (int)se.y - (int)ne.y);
      gy.z = (short)tap((int)sw.z - (int)nw.z, (int)s.z - (int)n.z, (int)se.z - (int)ne.z);
      gx.w = gy.w = 255;
    }
    P.gx[lv][i] = gx;
    P.gy[lv][i] = gy;
  }
}

struct ColourParams {
  Mat4 M;                      // world -> rgb camera
  float fx, fy, cx, cy;        // intr_rgb / 2^level
  int W, H;
  const uchar4* rgb; const short4* gx; const short4* gy;
  const int* countDev;         // noTotalPoints on the device (render-state counters), or null: countHost
  int countHost;
};

// interpolateBilinear: the right / lower taps are read only when the position is not on the pixel (bounds-safe at W-1, H-1)
template <class T>
__device__ inline float4 bilinear(const T* __restrict__ src, float px, float py, int W) {
  const int ix = (int)floorf(px), iy = (int)floorf(py);
  const float dx = px - (float)ix, dy = py - (float)iy;
  T a = src[ix + iy * W], b = {}, c = {}, d = {};
  if (dx != 0) b = src[(ix + 1) + iy * W];
  if (dy != 0) c = src[ix + (iy + 1) * W];
  if (dx != 0 && dy != 0) d = src[(ix + 1) + (iy + 1) * W];
  float4 r;
  r.x = ((float)a.x * (1.0f - dx) * (1.0f - dy) + (float)b.x * dx * (1.0f - dy) + (float)c.x * (1.0f - dx) * dy + (float)d.x * dx * dy);
  r.y = ((float)a.y * (1.0f - dx) * (1.0f - dy) + (float)b.y * dx * (1.0f - dy) + (float)c.y * (1.0f - dx) * dy + (float)d.y * dx * dy);
  r.z = ((float)a.z * (1.0f - dx) * (1.0f - dy) + (float)b.z * dx * (1.0f - dy) + (float)c.z * (1.0f - dx) * dy + (float)d.z * dx * dy);
  r.w = ((float)a.w * (1.0f - dx) * (1.0f - dy) + (float)b.w * dx * (1.0f - dy) + (float)c.w * (1.0f - dx) * dy + (float)d.w * dx * dy);
  return r;
}

// NP parameters (3: rotation only, the reference's startPara 3; 6: translation then rotation); GH: gradient / Hessian terms too
template <int NP, bool GH>
__global__ void __launch_bounds__(kGHThreads) colour_eval_kernel(const float4* __restrict__ locations, const float4* __restrict__ colours,
                                                                ColourParams p, GHBlockRecord* __restrict__ hostRec, unsigned int seq) {
  __shared__ double lds[kGHWaves][kGHValues];
  __shared__ int ldsCount[kGHWaves];
  constexpr int kStart = (NP == 3) ? 3 : 0;
  double acc[kGHValues];
#pragma unroll
  for (int i = 0; i < kGHValues; ++i) acc[i] = 0.0;
  int valid = 0;
  const int n = p.countDev ? *p.countDev : p.countHost;
  const float* m = p.M.m;
  for (int i = blockIdx.x * kGHThreads + threadIdx.x; i < n; i += gridDim.x * kGHThreads) {
    const float4 pt = locations[i], known = colours[i];
    const float cx = m[0] * pt.x + m[4] * pt.y + m[8] * pt.z + m[12] * pt.w;
    const float cy = m[1] * pt.x + m[5] * pt.y + m[9] * pt.z + m[13] * pt.w;
    const float cz = m[2] * pt.x + m[6] * pt.y + m[10] * pt.z + m[14] * pt.w;
    const float cw = m[3] * pt.x + m[7] * pt.y + m[11] * pt.z + m[15] * pt.w;
    if (cz <= 0) continue;
    const float u = p.fx * cx / cz + p.cx, v = p.fy * cy / cz + p.cy;
    // the reference's bounds test, written so that a NaN position fails it as well (the taps stay inside the level)
    if (!(u >= 0 && u <= (float)(p.W - 1) && v >= 0 && v <= (float)(p.H - 1))) continue;
    const float4 obs = bilinear(p.rgb, u, v, p.W);
    if (obs.w < 254.0f) continue;
    ++valid;
    const float ex = obs.x - 255.0f * known.x, ey = obs.y - 255.0f * known.y, ez = obs.z - 255.0f * known.z;
    acc[0] += (double)(ex * ex + ey * ey + ez * ez);
    if (GH) {
      const float4 gxo = bilinear(p.gx, u, v, p.W), gyo = bilinear(p.gy, u, v, p.W);
      const float dx = 2.0f * ex, dy = 2.0f * ey, dz = 2.0f * ez;   // 2 (obs - 255 known): the same float as 2.0f * (obs - 255 known)
      float d[NP][3];
#pragma unroll
      for (int para = 0, k = 0; para < NP; ++para) {
        float px, py, pz;
        switch (para + kStart) {
          case 0: px = cw; py = 0.0f; pz = 0.0f; break;
          case 1: px = 0.0f; py = cw; pz = 0.0f; break;
          case 2: px = 0.0f; py = 0.0f; pz = cw; break;
          case 3: px = 0.0f; py = -cz; pz = cy; break;
          case 4: px = cz; py = 0.0f; pz = -cx; break;
          default: px = -cy; py = cx; pz = 0.0f; break;
        }
        const float jx = p.fx * ((cz * px - pz * cx) / (cz * cz));
        const float jy = p.fy * ((cz * py - pz * cy) / (cz * cz));
        d[para][0] = jx * gxo.x + jy * gyo.x;
        d[para][1] = jx * gxo.y + jy * gyo.y;
        d[para][2] = jx * gxo.z + jy * gyo.z;
        acc[1 + para] += (double)(d[para][0] * dx + d[para][1] * dy + d[para][2] * dz);
#pragma unroll
        for (int col = 0; col <= para; ++col, ++k)
          acc[7 + k] += (double)(2.0f * (d[para][0] * d[col][0] + d[para][1] * d[col][1] + d[para][2] * d[col][2]));
      }
    }
  }
  double mine; int cnt;
  gh_block_reduce<(NP == 6) ? 3 : 1>(acc, valid, lds, ldsCount, mine, cnt);
  send_record<__HIP_MEMORY_SCOPE_SYSTEM>(hostRec + blockIdx.x, mine, cnt, seq);
}

}  // namespace itm

struct itm_colour_tracker : itm::GHHandle {
  itm::DeviceBuffer<void> pyramidMem;
  itm::ColourPyramid P = {};
  float intr[4] = {0, 0, 0, 0};    // intr_rgb of the last prepare
  itm::PinnedBuffer<int> totalHost;   // pinned: noTotalPoints copied from the render state (track_camera)
  int evaluations = 0;
};

namespace itm {

GHHandle* gh_handle(itm_colour_tracker* t) { return static_cast<GHHandle*>(t); }

static void colour_release(itm_colour_tracker* t) {
  t->ch.release();
  t->totalHost.reset(); t->pyramidMem.reset();
  t->P = ColourPyramid{};
}

static int colour_reserve(itm_colour_tracker* t, size_t pyramidBytes) {
  const int rc = t->ready([&] { colour_release(t); });
  if (rc) return rc;
  if (!t->totalHost) {
    const hipError_t e = t->totalHost.alloc(1, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) { colour_release(t); return hip_fail(e, "colour tracker buffers", __FILE__, __LINE__); }
  }
  const hipError_t e = t->pyramidMem.reserve(pyramidBytes);
  if (e != hipSuccess) { colour_release(t); return hip_fail(e, "colour tracker pyramid", __FILE__, __LINE__); }
  return ITM_OK;
}

static int colour_prepare(itm_colour_tracker* t, const itm_view* view, int levels, hipStream_t st) {
  if (!view || !view->rgb) return set_error(ITM_ERR_INVALID, "colour tracker: null view or rgb image");
  if (levels < 1 || levels > kColourMaxLevels) return set_error(ITM_ERR_INVALID, "colour tracker: 1..8 hierarchy levels");
  if (view->w_rgb <= 0 || view->h_rgb <= 0 || (view->w_rgb >> (levels - 1)) < 1 || (view->h_rgb >> (levels - 1)) < 1)
    return set_error(ITM_ERR_INVALID, "colour tracker: rgb image too small for the hierarchy");
  ColourPyramid P = {};
  P.levels = levels;
  size_t bytes = 0, off[kColourMaxLevels];
  for (int l = 0; l < levels; ++l) {
    P.w[l] = view->w_rgb >> l; P.h[l] = view->h_rgb >> l;   // floor halves, as FilterSubsample's ChangeDims
    off[l] = bytes;
    bytes += ((size_t)P.w[l] * P.h[l] * (4 + 8 + 8) + 255) & ~(size_t)255;
  }
  int rc = colour_reserve(t, bytes);
  if (rc) return rc;
  char* base = (char*)t->pyramidMem.get();
  for (int l = 0; l < levels; ++l) {
    const size_t n = (size_t)P.w[l] * P.h[l];
    P.rgb[l] = (uchar4*)(base + off[l]);
    P.gx[l] = (short4*)(base + off[l] + 4 * n);
    P.gy[l] = (short4*)(base + off[l] + 12 * n);
  }
  // level 0 copied and up to four coarser levels per launch (one launch for the default five levels)
  for (int first = 0; first == 0 || first < levels - 1; first += 4) {
    const int count = std::min(4, levels - 1 - first);
    const dim3 grid((P.w[first] + 15) / 16, (P.h[first] + 15) / 16);
    colour_pyramid_kernel<<<grid, 256, 0, st>>>(first == 0 ? (const uchar4*)view->rgb : P.rgb[first], P, first, count,
                                                first == 0 ? P.rgb[0] : nullptr);
    ITM_LAUNCH_CHECK();
  }
  const dim3 ggrid((unsigned)std::min((P.w[0] * P.h[0] + 255) / 256, 1024), levels);
  colour_gradient_kernel<<<ggrid, 256, 0, st>>>(P);
  ITM_LAUNCH_CHECK();
  t->P = P;
  memcpy(t->intr, view->intr_rgb, sizeof t->intr);
  return ITM_OK;
}

// One pass over the point cloud at `pose` (float matrix): f and the valid count, the gradient / Hessian too when gh.
static int colour_evaluate(itm_colour_tracker* t, int level, const float* locations, const float* colours, const int* countDev,
                           int countHost, const float pose[16], int mode, bool gh, itm_colour_eval* out, hipStream_t st) {
  memset(out, 0, sizeof *out);
  if (level < 0 || level >= t->P.levels) return set_error(ITM_ERR_INVALID, "colour tracker: level not prepared");
  if (mode < ITM_TRACKER_ITERATION_ROTATION || mode > ITM_TRACKER_ITERATION_BOTH)
    return set_error(ITM_ERR_INVALID, "colour tracker: iteration type must be ROTATION, TRANSLATION or BOTH");
  if (!locations || !colours) return set_error(ITM_ERR_INVALID, "colour tracker: null point cloud");
  ColourParams p;
  memcpy(p.M.m, pose, 64);
  const float scale = (float)(1 << level);
  p.fx = t->intr[0] / scale; p.fy = t->intr[1] / scale; p.cx = t->intr[2] / scale; p.cy = t->intr[3] / scale;
  p.W = t->P.w[level]; p.H = t->P.h[level];
  p.rgb = t->P.rgb[level]; p.gx = t->P.gx[level]; p.gy = t->P.gy[level];
  p.countDev = countDev; p.countHost = countHost;
  const int np = colour_num_para(mode);
  const float4* loc = (const float4*)locations; const float4* col = (const float4*)colours;
  const dim3 grid(kGHGroups);
  double sums[kGHValues];
  int valid = 0;
  const int rc = t->evaluate(kGHGroups, st, [&](GHBlockRecord* rec, unsigned int seq) {
    if (np == 3) {
      if (gh) colour_eval_kernel<3, true><<<grid, kGHThreads, 0, st>>>(loc, col, p, rec, seq);
      else colour_eval_kernel<3, false><<<grid, kGHThreads, 0, st>>>(loc, col, p, rec, seq);
    } else {
      if (gh) colour_eval_kernel<6, true><<<grid, kGHThreads, 0, st>>>(loc, col, p, rec, seq);
      else colour_eval_kernel<6, false><<<grid, kGHThreads, 0, st>>>(loc, col, p, rec, seq);
    }
    return ITM_OK;
  }, sums, &valid);
  if (rc) return rc;
  // the launch has finished (its records are in): the count it read is in place as well
  const int total = countDev ? *(volatile int*)t->totalHost.get() : countHost;
  // F_oneLevel / G_oneLevel scaling (MY_INF is the integer 0x7f800000 converted to float)
  out->noValidPoints = valid;
  out->numPara = np;
  float sc;
  if (valid == 0) { out->f = (float)0x7f800000 * 1.0f; sc = 1.0f; }
  else { sc = (float)total / (float)valid; out->f = (float)sums[0] * sc; }
  if (gh) unpack_gh(sums, np, np, sc, out->nabla, out->hessian);
  return ITM_OK;
}

static int colour_track_camera(itm_colour_tracker* t, const itm_tracker_config* cfg, const itm_view* view, const itm_render_state* rs,
                               const float* locations, const float* colours, int noTotalPoints, float M_d_out[16], hipStream_t st) {
  if (!cfg || !view || !M_d_out) return set_error(ITM_ERR_INVALID, "null argument");
  if (!rs && noTotalPoints < 0) return set_error(ITM_ERR_INVALID, "negative point count");
  if (cfg->noHierarchyLevels < 1 || cfg->noHierarchyLevels > kColourMaxLevels) return set_error(ITM_ERR_INVALID, "colour tracker: 1..8 hierarchy levels");
  for (int l = 0; l < cfg->noHierarchyLevels; ++l) {
    const int m = cfg->trackingRegime[l];
    if (m < ITM_TRACKER_ITERATION_ROTATION || m > ITM_TRACKER_ITERATION_BOTH)
      return set_error(ITM_ERR_INVALID, "colour tracker: every level needs ROTATION, TRANSLATION or BOTH (NONE leaves the step undefined)");
  }
  if (!locations || !colours) return set_error(ITM_ERR_INVALID, "colour tracker: null point cloud");
  int rc = colour_prepare(t, view, cfg->noHierarchyLevels, st);
  if (rc) return rc;
  // the point count stays on the device for the kernels; the host's copy (for the scaling) travels with the first evaluation's stream
  const int* countDev = rs ? &rs->counters->noTotalPoints : nullptr;
  if (countDev) ITM_HIP(hipMemcpyAsync(t->totalHost, countDev, sizeof(int), hipMemcpyDeviceToHost, st));
  auto evaluate = [&](int level, int mode, ColourPoint& x) -> int {
    float M[16];
    se3::to_matrix(x.pose, M);
    itm_colour_eval e;
    const int r = colour_evaluate(t, level, locations, colours, countDev, noTotalPoints, M, mode, true, &e, st);
    if (r) return r;
    const int n = e.numPara;
    x.f = (double)e.f;
    for (int i = 0; i < n; ++i) x.g[i] = (double)e.nabla[i];
    for (int i = 0; i < n * n; ++i) x.H[i] = (double)e.hessian[i];
    return ITM_OK;
  };
  return colour_track(cfg, view->M_d, view->rgb_to_depth, view->rgb_to_depth_inv, M_d_out, evaluate, &t->evaluations);
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_colour_tracker_create(itm_colour_tracker** out) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  *out = new (std::nothrow) itm_colour_tracker();
  return *out ? ITM_OK : set_error(ITM_ERR_DEVICE, "out of host memory");
}

int itm_colour_tracker_destroy(itm_colour_tracker* t) {
  if (!t) return ITM_OK;
  { std::lock_guard<std::mutex> g(t->mu); colour_release(t); }
  delete t;
  return ITM_OK;
}

int itm_colour_tracker_prepare(itm_colour_tracker* t, const itm_view* view, int levels, itm_stream stream) {
  if (!t) return set_error(ITM_ERR_INVALID, "null tracker");
  std::lock_guard<std::mutex> g(t->mu);
  return colour_prepare(t, view, levels, as_stream(stream));
}

int itm_colour_tracker_read_level(itm_colour_tracker* t, int level, uint8_t* rgb, int16_t* gx, int16_t* gy, int* w, int* h, itm_stream stream) {
  if (!t) return set_error(ITM_ERR_INVALID, "null tracker");
  std::lock_guard<std::mutex> g(t->mu);
  if (level < 0 || level >= t->P.levels) return set_error(ITM_ERR_INVALID, "colour tracker: level not prepared");
  const size_t n = (size_t)t->P.w[level] * t->P.h[level];
  const hipStream_t st = as_stream(stream);
  if (rgb) ITM_HIP(hipMemcpyAsync(rgb, t->P.rgb[level], n * 4, hipMemcpyDeviceToHost, st));
  if (gx) ITM_HIP(hipMemcpyAsync(gx, t->P.gx[level], n * 8, hipMemcpyDeviceToHost, st));
  if (gy) ITM_HIP(hipMemcpyAsync(gy, t->P.gy[level], n * 8, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (w) *w = t->P.w[level];
  if (h) *h = t->P.h[level];
  return ITM_OK;
}

int itm_colour_tracker_evaluate(itm_colour_tracker* t, int level, const float* locations, const float* colours, int noTotalPoints,
                                const float pose[16], int iterationType, int wantGH, itm_colour_eval* out, itm_stream stream) {
  if (!t || !pose || !out) return set_error(ITM_ERR_INVALID, "null argument");
  if (noTotalPoints < 0) return set_error(ITM_ERR_INVALID, "negative point count");
  std::lock_guard<std::mutex> g(t->mu);
  return colour_evaluate(t, level, locations, colours, nullptr, noTotalPoints, pose, iterationType, wantGH != 0, out, as_stream(stream));
}

int itm_colour_tracker_track_camera(itm_colour_tracker* t, const itm_tracker_config* cfg, const itm_view* view, const itm_render_state* rs,
                                    const float* locations, const float* colours, int noTotalPoints, float M_d_out[16], itm_stream stream) {
  if (!t) return set_error(ITM_ERR_INVALID, "null tracker");
  std::lock_guard<std::mutex> g(t->mu);
  return colour_track_camera(t, cfg, view, rs, locations, colours, noTotalPoints, M_d_out, as_stream(stream));
}

int itm_colour_tracker_evaluations(const itm_colour_tracker* t, int* out) {
  if (!t || !out) return set_error(ITM_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> g(t->mu);
  *out = t->evaluations;
  return ITM_OK;
}

}  // extern "C"
