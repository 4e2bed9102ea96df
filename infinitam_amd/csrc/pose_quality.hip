// pose_quality.hip -- a depth image under a pose, judged against the fused TSDF (include/itm_hip.h: itm_pose_quality_*): the counts
// behind the GOOD / POOR / FAILED tracking verdict.  The reference at this revision has no such judgement; the sequential definition
// in the header is the specification and tests/pose_quality_terms.py its restatement.
//
// Reads restated (every value through the functions the ray cast and the scene queries use):
//   readFromSDF_float_interpolated / _uninterpolated   DeviceAgnostic/ITMRepresentationAccess.h:144-185   (volume_device.h: Corners)
//   readVoxel: an absent voxel reads TVoxel()          :85-142                                            (locate_voxel)
//
// MI355X design.  ONE launch per evaluation: a lane back-projects its pixel, transforms it, gathers the trilinear cell and the nearest
// voxel (Corners::fetch: the up-to-eight blocks resolved together, then eight loads in flight; the nearest voxel is one of the eight
// corners), reads that voxel's weight (locate_voxel through the block the fetch left in the lane's cache), classifies and accumulates
// four doubles and a count; no per-point buffer exists between these steps.  The reduction is gh_reduce.h's: DPP row sums per wave,
// the four waves in order, one tagged record per workgroup into page-locked host memory, the records added by the host in the fixed
// segment order -- so the counts (exact as doubles) and the two sums reach the caller without a stream synchronise, the same bits
// on every call.  A wave covers an 8 x 8 pixel tile: neighbouring pixels land in the same or adjacent voxel blocks, and a tile's
// footprint in the volume is a patch instead of a strip (ITM_DEBUG_POSE_QUALITY_ROWS: 64 consecutive pixels of a row instead; 640 x 480
// on the benchmark scene: 11.9 us a launch against 12.5 us, 24.2 us a call against 25.0 us, profiles/pose_quality_bench.json).
// Every loop is wave-uniform: a lane without a pixel, with a hole or with a point outside the query limits gathers at voxel position
// (0, 0, 0) and drops the values, as an invalid point of itm_scene_query_points does.
#include <climits>
#include <cstring>
#include <mutex>
#include <new>

#include "itm_internal.h"
#include "gh_reduce.h"
#include "volume_device.h"

namespace itm {

constexpr float kQualityPointLimit = 262136.0f;      // itm_scene_query_points' limit on |p| in voxels (query.hip: kPointLimit)

struct PoseQualityParams {
  Mat4 invM;                   // camera -> world
  float fx, fy, cx, cy;
  float voxelSize, mu, inlierDistance;
  int minWeight;
  int w, h;
};

// acc / record layout: [0] noKnown, [1] noInliers, [2] sumSqKnown, [3] sumSqInliers (the values gh_block_reduce<1> adds up); the
// record's count is noValid
template <class VX, bool DENSE, bool TILES>
__global__ void __launch_bounds__(kGHThreads) pose_quality_kernel(VolumeView vol, const float* __restrict__ depth, PoseQualityParams p,
                                                                 float* __restrict__ residuals, GHBlockRecord* __restrict__ hostRec, unsigned int seq) {
  __shared__ double lds[kGHWaves][kGHValues];
  __shared__ int ldsCount[kGHWaves];
  double acc[kGHValues];
#pragma unroll
  for (int i = 0; i < kGHValues; ++i) acc[i] = 0.0;
  int valid = 0;
  const int lane = threadIdx.x & 63;
  const int unitsX = TILES ? (p.w + 7) >> 3 : 0, unitsY = TILES ? (p.h + 7) >> 3 : 0;
  const int pixels = p.w * p.h;
  const int units = TILES ? unitsX * unitsY : (pixels + 63) >> 6;      // what one wave covers at a time
  const float* m = p.invM.m;
  for (int u = blockIdx.x * kGHWaves + (int)(threadIdx.x >> 6); u < units; u += gridDim.x * kGHWaves) {      // (wave-uniform)
    int x, y;
    bool live;
    if (TILES) {
      x = (u % unitsX) * 8 + (lane & 7); y = (u / unitsX) * 8 + (lane >> 3);
      live = x < p.w && y < p.h;
    } else {
      const int i = u * 64 + lane;
      live = i < pixels;
      x = live ? i % p.w : 0; y = live ? i / p.w : 0;
    }
    const int pix = live ? y * p.w + x : 0;
    const float d = depth[pix];
    const bool some = live && d > 0.0f;            // false for -1, 0 and NaN: NONE
    const float cxm = d * (((float)x - p.cx) / p.fx), cym = d * (((float)y - p.cy) / p.fy);
    const float wx = ((m[0] * cxm + m[4] * cym) + m[8] * d) + m[12];
    const float wy = ((m[1] * cxm + m[5] * cym) + m[9] * d) + m[13];
    const float wz = ((m[2] * cxm + m[6] * cym) + m[10] * d) + m[14];
    float px = wx / p.voxelSize, py = wy / p.voxelSize, pz = wz / p.voxelSize;
    const bool inside = some && (fabsf(px) < kQualityPointLimit) && (fabsf(py) < kQualityPointLimit) && (fabsf(pz) < kQualityPointLimit);
    if (!inside) px = py = pz = 0.0f;
    BlockCache cache;
    Corners<VX, DENSE> cn;
    cn.fetch(vol, px, py, pz, cache);
    bool found = false;
    (void)cn.nearest(px, py, pz, found);
    // the stored voxel itself: the mirror holds the sdf alone
    const long long a = locate_voxel<DENSE>(vol, (int)round_ref(px), (int)round_ref(py), (int)round_ref(pz), cache);
    const typename VX::Reg reg = VX::load(vol.vba, a < 0 ? (size_t)0 : (size_t)a);
    const int weight = a < 0 ? 0 : VX::w_depth(reg);
    const float r = cn.trilinear() * p.mu;
    const bool known = inside && found && weight >= p.minWeight;
    const bool inlier = known && fabsf(r) <= p.inlierDistance;
    const double rr = (double)r * (double)r;
    valid += some ? 1 : 0;
    acc[0] += known ? 1.0 : 0.0;
    acc[1] += inlier ? 1.0 : 0.0;
    acc[2] += known ? rr : 0.0;
    acc[3] += inlier ? rr : 0.0;
    if (residuals && live) residuals[pix] = known ? r : (some ? ITM_POSE_QUALITY_UNKNOWN : ITM_POSE_QUALITY_NONE);
  }
  double mine; int cnt;
  gh_block_reduce<1>(acc, valid, lds, ldsCount, mine, cnt);
  send_record<__HIP_MEMORY_SCOPE_SYSTEM>(hostRec + blockIdx.x, mine, cnt, seq);
}

// what is wrong with a configuration, or nullptr
static const char* quality_config_fault(const itm_pose_quality_config* c) {
  auto fraction = [](float f) { return f >= 0.0f && f <= 1.0f; };      // false for NaN
  if (!(c->inlierDistance > 0.0f)) return "pose quality: inlierDistance must be positive";
  if (c->minWeight < 1) return "pose quality: minWeight < 1";
  if (!fraction(c->minValidFraction) || !fraction(c->failOverlap) || !fraction(c->poorOverlap) || !fraction(c->failInliers) || !fraction(c->goodInliers))
    return "pose quality: a fraction lies outside [0, 1]";
  if (c->failOverlap > c->poorOverlap) return "pose quality: failOverlap > poorOverlap";
  if (c->failInliers > c->goodInliers) return "pose quality: failInliers > goodInliers";
  return nullptr;
}

}  // namespace itm

using namespace itm;

struct itm_pose_quality_handle : itm::GHHandle {};      // the pinned records of this handle's launches

namespace itm {
GHHandle* gh_handle(itm_pose_quality_handle* q) { return static_cast<GHHandle*>(q); }
}  // namespace itm

extern "C" {

int itm_pose_quality_default_config(float mu, itm_pose_quality_config* cfg) {
  if (!cfg) return set_error(ITM_ERR_INVALID, "null argument");
  if (!(mu > 0.0f)) return set_error(ITM_ERR_INVALID, "pose quality: mu must be positive");
  // POLICY, not measurement: chosen on the synthetic sphere-and-wall scene of the tests, never tuned on sensor data (include/itm_hip.h)
  cfg->inlierDistance = 0.5f * mu;
  cfg->minWeight = 1;
  cfg->minValidFraction = 0.05f;
  cfg->failOverlap = 0.10f; cfg->poorOverlap = 0.30f;
  cfg->failInliers = 0.50f; cfg->goodInliers = 0.90f;
  return ITM_OK;
}

int itm_pose_quality_verdict(const itm_pose_quality* s, const itm_pose_quality_config* cfg, int32_t* result) {
  if (!s || !cfg || !result) return set_error(ITM_ERR_INVALID, "null argument");
  if (const char* why = quality_config_fault(cfg)) return set_error(ITM_ERR_INVALID, why);
  const double pixels = (double)s->noPixels, valid = (double)s->noValid, known = (double)s->noKnown, inliers = (double)s->noInliers;
  if (valid < (double)cfg->minValidFraction * pixels || known < (double)cfg->failOverlap * valid || inliers < (double)cfg->failInliers * known || s->noKnown == 0)
    *result = ITM_TRACKING_FAILED;
  else if (known < (double)cfg->poorOverlap * valid || inliers < (double)cfg->goodInliers * known)
    *result = ITM_TRACKING_POOR;
  else
    *result = ITM_TRACKING_GOOD;
  return ITM_OK;
}

int itm_pose_quality_create(itm_pose_quality_handle** out) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  *out = new (std::nothrow) itm_pose_quality_handle();
  return *out ? ITM_OK : set_error(ITM_ERR_DEVICE, "out of host memory");
}

int itm_pose_quality_destroy(itm_pose_quality_handle* q) {
  if (!q) return ITM_OK;
  { std::lock_guard<std::mutex> g(q->mu); q->ch.release(); }
  delete q;
  return ITM_OK;
}

int itm_pose_quality_evaluate(itm_pose_quality_handle* q, const itm_scene* s, const itm_view* view, const itm_pose_quality_config* cfg, itm_pose_quality* out,
                              float* residuals_dev, itm_stream stream) {
  if (!q || !s || !view || !cfg || !out || !view->depth) return set_error(ITM_ERR_INVALID, "null argument");
  if (view->w < 1 || view->h < 1 || (long long)view->w * view->h > (long long)INT_MAX - 64) return set_error(ITM_ERR_INVALID, "pose quality: empty or oversized depth image");
  if (const char* why = quality_config_fault(cfg)) return set_error(ITM_ERR_INVALID, why);
  PoseQualityParams p;
  if (!invert4(view->M_d, p.invM.m)) return set_error(ITM_ERR_INVALID, "pose matrix is singular");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const int pixels = view->w * view->h;
  // the residual image may be read by a recorded (not yet launched) call of another scene
  if (residuals_dev) { const int rc = flush_overlapping(residuals_dev, (size_t)pixels * 4, st); if (rc) return rc; }
  std::lock_guard<std::mutex> lock(q->mu);
  { const int rc = q->ready([&] { q->ch.release(); }); if (rc) return rc; }
  p.fx = view->intr_d[0]; p.fy = view->intr_d[1]; p.cx = view->intr_d[2]; p.cy = view->intr_d[3];
  p.voxelSize = s->prm.voxelSize; p.mu = s->prm.mu; p.inlierDistance = cfg->inlierDistance; p.minWeight = cfg->minWeight;
  p.w = view->w; p.h = view->h;
  const bool tiles = debug_value(ITM_DEBUG_POSE_QUALITY_ROWS) == 0;
  const long long units = tiles ? (long long)((view->w + 7) >> 3) * ((view->h + 7) >> 3) : ((long long)pixels + 63) >> 6;
  const long long groups = (units + kGHWaves - 1) / kGHWaves;
  const int grid = (int)(groups < kGHGroups ? groups : kGHGroups);
  const VolumeView vol = make_volume(s);
  double sums[kGHValues];
  int valid = 0;
  const int rc = q->evaluate((size_t)grid, st, [&](GHBlockRecord* rec, unsigned int seq) {
    return dispatch_volume(s, [&](auto vx, auto dense) {
      using VX = decltype(vx);
      if (tiles) pose_quality_kernel<VX, dense.value, true><<<grid, kGHThreads, 0, st>>>(vol, view->depth, p, residuals_dev, rec, seq);
      else pose_quality_kernel<VX, dense.value, false><<<grid, kGHThreads, 0, st>>>(vol, view->depth, p, residuals_dev, rec, seq);
      return ITM_OK;
    });
  }, sums, &valid);
  if (rc) return rc;
  out->noPixels = pixels; out->noValid = valid;
  out->noKnown = (int32_t)sums[0]; out->noInliers = (int32_t)sums[1];
  out->sumSqKnown = sums[2]; out->sumSqInliers = sums[3];
  return ITM_OK;
}

}  // extern "C"
