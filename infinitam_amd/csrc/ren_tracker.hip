// ren_tracker.hip -- Ren SDF tracker: registers the depth image of a view directly against the fused TSDF volume.
//
// Reference behaviour:
//   unprojectPtWithIntrinsic, computePerPixelEnergy, computeDDT, computePerPixelJacobian   DeviceAgnostic/ITMRenTracker.h
//   ITMRenTracker_CPU::UnprojectDepthToCam / F_oneLevel / G_oneLevel                       DeviceSpecific/CPU/ITMRenTracker_CPU.cpp
//   readFromSDF_float_uninterpolated / readVoxel                                           DeviceAgnostic/ITMRepresentationAccess.h
//   ITMRenTracker::TrackCamera / ComputeSingleStep / GetMFromParam                         Engine/ITMRenTracker.cpp (host loop: ren_solver.h)
//
// Device part: one launch unprojects the depth image (level 0 only: the reference's level 1 is never read); one launch per
// evaluation, one lane per point, reads the scene through the shared voxel access (volume_device.h: sdf mirror, block directory,
// table walk, dense array -- the same values on every path) and computes the energy and -- in the same pass -- the Jacobian terms with
// the reference's float operations (no contraction: the valid count is exact), reduced with the fixed-order double tree of
// gh_reduce.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

#include "itm_internal.h"
#include "gh_reduce.h"
#include "volume_device.h"
#include "ren_solver.h"
#include "se3.h"

namespace itm {

constexpr float kRenDTune = 6.0f;   // DTUNE: sigma of the basin of attraction

// UnprojectDepthToCam: (x z, y z, z) through ooIntrinsics = (1/fx, 1/fy, -cx/fx, -cy/fy); (0, 0, 0, -1) where depth <= 0
__global__ void __launch_bounds__(256) ren_unproject_kernel(const float* __restrict__ depth, float4* __restrict__ out, int W, int H,
                                                            float ox, float oy, float oz, float ow) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W * H) return;
  const int x = i % W, y = i / W;
  const float z = depth[i];
  float4 r = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  if (z > 0.0f) {
    const float ix = (float)x * z, iy = (float)y * z;
    r = make_float4(ox * ix + oz * z, oy * iy + ow * z, z, 1.0f);
  }
  out[i] = r;
}

struct RenParams {
  Mat4 invM;                   // camera -> world
  float oneOverVoxel;
  int n;
};

// GH: the Jacobian terms too (G_oneLevel); f (F_oneLevel's sum of per-point energies) always
template <class VX, bool DENSE, bool GH>
__global__ void __launch_bounds__(kGHThreads) ren_eval_kernel(VolumeView vol, const float4* __restrict__ pts, RenParams p,
                                                             GHBlockRecord* __restrict__ hostRec, unsigned int seq) {
  __shared__ double lds[kGHWaves][kGHValues];
  __shared__ int ldsCount[kGHWaves];
  double acc[kGHValues];
#pragma unroll
  for (int i = 0; i < kGHValues; ++i) acc[i] = 0.0;
  int valid = 0;
  const float* m = p.invM.m;
  BlockCache cache;
  for (int i = blockIdx.x * kGHThreads + threadIdx.x; i < p.n; i += gridDim.x * kGHThreads) {
    const float4 in = pts[i];
    if (!(in.w > -1.0f)) continue;            // F: w > -1; G skips w == -1 (the unprojection writes 1 or -1)
    const float cx = m[0] * in.x + m[4] * in.y + m[8] * in.z + m[12] * in.w;
    const float cy = m[1] * in.x + m[5] * in.y + m[9] * in.z + m[13] * in.w;
    const float cz = m[2] * in.x + m[6] * in.y + m[10] * in.z + m[14] * in.w;
    const float px = cx * p.oneOverVoxel, py = cy * p.oneOverVoxel, pz = cz * p.oneOverVoxel;
    const int ix = (int)round_ref(px), iy = (int)round_ref(py), iz = (int)round_ref(pz);
    bool found;
    const float dt = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix, iy, iz, found, cache));
    if (dt == 1.0f) continue;                 // no energy, no Jacobian (a voxel that was not found reads 1)
    const float expdt = expf(-dt * kRenDTune);
    acc[0] += (double)(4.0f * expdt / ((expdt + 1.0f) * (expdt + 1.0f)));
    if (GH) {
      if (!found) continue;
      // computeDDT: the six axis neighbours of the rounded position, all found and != 1 (loads issued together)
      bool f0, f1, f2, f3, f4, f5;
      const float a0 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix + 1, iy, iz, f0, cache));
      const float a1 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix - 1, iy, iz, f1, cache));
      const float a2 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix, iy + 1, iz, f2, cache));
      const float a3 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix, iy - 1, iz, f3, cache));
      const float a4 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix, iy, iz + 1, f4, cache));
      const float a5 = VX::to_float(read_raw_sdf<VX, DENSE>(vol, ix, iy, iz - 1, f5, cache));
      const bool ok = f0 && f1 && f2 && f3 && f4 && f5 && a0 != 1.0f && a1 != 1.0f && a2 != 1.0f && a3 != 1.0f && a4 != 1.0f && a5 != 1.0f;
      if (!ok) continue;
      const float deto = expdt + 1.0f;
      const float prefix = 4.0f * kRenDTune * (2.0f * expf(-dt * 2.0f * kRenDTune) / (deto * deto * deto) - expdt / (deto * deto));
      const float dx = (a0 - a1) * 0.5f * prefix, dy = (a2 - a3) * 0.5f * prefix, dz = (a4 - a5) * 0.5f * prefix;
      float j[6];
      j[0] = dx; j[1] = dy; j[2] = dz;
      j[3] = 4.0f * (dz * cy - dy * cz);
      j[4] = 4.0f * (dx * cz - dz * cx);
      j[5] = 4.0f * (dy * cx - dx * cy);
      ++valid;
#pragma unroll
      for (int r = 0, k = 0; r < 6; ++r) {
        acc[1 + r] -= (double)j[r];
#pragma unroll
        for (int c = 0; c <= r; ++c, ++k) acc[7 + k] += (double)(j[r] * j[c]);
      }
    }
  }
  double mine; int cnt;
  gh_block_reduce<GH ? 3 : 1>(acc, valid, lds, ldsCount, mine, cnt);
  send_record<__HIP_MEMORY_SCOPE_SYSTEM>(hostRec + blockIdx.x, mine, cnt, seq);
}

}  // namespace itm

struct itm_ren_tracker : itm::GHHandle {
  itm::DeviceBuffer<float4> points;
  int w = 0, h = 0;                // size of the last prepared depth image (0: nothing prepared)
};

namespace itm {

GHHandle* gh_handle(itm_ren_tracker* t) { return static_cast<GHHandle*>(t); }

static void ren_release(itm_ren_tracker* t) {
  t->ch.release();
  t->points.reset();
  t->w = t->h = 0;
}

static int ren_prepare(itm_ren_tracker* t, const itm_view* view, hipStream_t st) {
  if (!view || !view->depth) return set_error(ITM_ERR_INVALID, "Ren tracker: null view or depth image");
  if (view->w <= 0 || view->h <= 0) return set_error(ITM_ERR_INVALID, "Ren tracker: empty depth image");
  int rc = t->ready([&] { ren_release(t); });
  if (rc) return rc;
  const hipError_t e = t->points.reserve((size_t)view->w * view->h);
  if (e != hipSuccess) { ren_release(t); return hip_fail(e, "Ren tracker points", __FILE__, __LINE__); }
  // the view's depth image may be the target of a recorded (not yet launched) engine call
  rc = flush_overlapping(view->depth, (size_t)view->w * view->h * 4, st);
  if (rc) return rc;
  const float* in = view->intr_d;
  const float ox = 1.0f / in[0], oy = 1.0f / in[1];
  const float oz = -in[2] * ox, ow = -in[3] * oy;
  const int P = view->w * view->h;
  ren_unproject_kernel<<<(P + 255) / 256, 256, 0, st>>>(view->depth, t->points, view->w, view->h, ox, oy, oz, ow);
  ITM_LAUNCH_CHECK();
  t->w = view->w; t->h = view->h;
  return ITM_OK;
}

// One pass over the prepared points at the float inverse pose `invM`: f, and with gh the gradient, Hessian and valid count.
static int ren_evaluate(itm_ren_tracker* t, const itm_scene* s, const float invM[16], bool gh, itm_ren_eval* out, hipStream_t st) {
  memset(out, 0, sizeof *out);
  if (t->w <= 0) return set_error(ITM_ERR_INVALID, "Ren tracker: no depth image prepared");
  RenParams p;
  memcpy(p.invM.m, invM, 64);
  p.oneOverVoxel = 1.0f / s->prm.voxelSize;
  p.n = t->w * t->h;
  const VolumeView vol = make_volume(s);
  double sums[kGHValues];
  int valid = 0;
  const int rc = t->evaluate(kGHGroups, st, [&](GHBlockRecord* rec, unsigned int seq) {
    return dispatch_volume(s, [&](auto vx, auto dense) {
      using VX = decltype(vx);
      if (gh) ren_eval_kernel<VX, dense.value, true><<<kGHGroups, kGHThreads, 0, st>>>(vol, t->points, p, rec, seq);
      else ren_eval_kernel<VX, dense.value, false><<<kGHGroups, kGHThreads, 0, st>>>(vol, t->points, p, rec, seq);
      return ITM_OK;
    });
  }, sums, &valid);
  if (rc) return rc;
  out->f = -(float)sums[0];
  if (gh) {
    out->noValidPoints = valid;
    unpack_gh(sums, 6, 6, 1.0f, out->nabla, out->hessian);
  }
  return ITM_OK;
}

static int ren_track_camera(itm_ren_tracker* t, const itm_scene* s, const itm_view* view, float M_d_out[16], int* evaluations, hipStream_t st) {
  if (!view || !M_d_out) return set_error(ITM_ERR_INVALID, "null argument");
  int rc = ren_prepare(t, view, st);
  if (rc) return rc;
  int n = 0;
  rc = ren_track(view->M_d, M_d_out, [&](RenPoint& x) -> int {
    itm_ren_eval e;
    const int r = ren_evaluate(t, s, x.invM, true, &e, st);
    if (r) return r;
    x.f = e.f;
    memcpy(x.g, e.nabla, sizeof x.g);
    memcpy(x.H, e.hessian, sizeof x.H);
    return ITM_OK;
  }, &n);
  if (rc == ITM_ERR_INVALID) return set_error(rc, "Ren tracker: pose matrix is singular");
  if (evaluations) *evaluations = n;
  return rc;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_ren_tracker_create(itm_ren_tracker** out) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  *out = new (std::nothrow) itm_ren_tracker();
  return *out ? ITM_OK : set_error(ITM_ERR_DEVICE, "out of host memory");
}

int itm_ren_tracker_destroy(itm_ren_tracker* t) {
  if (!t) return ITM_OK;
  { std::lock_guard<std::mutex> g(t->mu); ren_release(t); }
  delete t;
  return ITM_OK;
}

int itm_ren_tracker_prepare(itm_ren_tracker* t, const itm_view* view, float* points_host, itm_stream stream) {
  if (!t) return set_error(ITM_ERR_INVALID, "null tracker");
  std::lock_guard<std::mutex> g(t->mu);
  const hipStream_t st = as_stream(stream);
  const int rc = ren_prepare(t, view, st);
  if (rc || !points_host) return rc;
  ITM_HIP(hipMemcpyAsync(points_host, t->points, (size_t)t->w * t->h * sizeof(float4), hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

int itm_ren_tracker_evaluate(itm_ren_tracker* t, const itm_scene* scene, const float invM[16], int wantG, itm_ren_eval* out,
                             itm_stream stream) {
  if (!t || !scene || !invM || !out) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = enter_scene(scene, nullptr); if (rc) return rc; }
  std::lock_guard<std::mutex> g(t->mu);
  return ren_evaluate(t, scene, invM, wantG != 0, out, as_stream(stream));
}

int itm_ren_tracker_track_camera(itm_ren_tracker* t, const itm_scene* scene, const itm_view* view, float M_d_out[16], int* evaluations,
                                 itm_stream stream) {
  if (!t || !scene) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = enter_scene(scene, nullptr); if (rc) return rc; }
  std::lock_guard<std::mutex> g(t->mu);
  return ren_track_camera(t, scene, view, M_d_out, evaluations, as_stream(stream));
}

}  // extern "C"
