// align.hip -- scene alignment (include/itm_hip.h: itm_scene_band_samples, itm_aligner_*): the rigid pose between sdf samples and a
// TSDF scene, refined on the GPU.  The reference has no counterpart; what is restated from it is the voxel read alone:
//   readVoxel / readFromSDF_float_interpolated   DeviceAgnostic/ITMRepresentationAccess.h:85-185   (volume_device.h: Corners)
// Host loop: align_solver.h.
//
// MI355X design.
// Band samples: both index types are one ordered compaction over a linear range (ordered_device.h) -- dense: the voxel index; hash:
// slot * 512 + voxel, so a chunk of 2048 elements is four table slots and each of a workgroup's four waves has ONE slot: the entry is
// a wave-uniform load, a wave without a block leaves with its count 0, and a lane's eight elements are one x-row of its block (one
// 32 .. 96-byte run of voxels).  A count pass leaves one count per chunk, one workgroup turns them into chunk bases (carry_scan), a
// fill pass repeats the test and writes at base + workgroup scan: ascending order without a sort or an atomic.
// Evaluation: one lane per sample, kGHThreads lanes per workgroup, at most kGHGroups workgroups, grid-stride (ren_eval_kernel's
// shape).  Band samples arrive block by block, so neighbouring lanes read neighbouring cells: the eight corner loads of Corners::fetch
// -- issued together, from the sdf mirror on the default path -- mostly hit lines a neighbour fetched.  Cost, gradient and the packed
// Hessian are 28 double accumulators per lane, added over the workgroup in the fixed order of gh_reduce.h and sent as one tagged
// record to the handle's own channel: no stream synchronise, the same bits on every run and path.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>

#include "itm_internal.h"
#include "gh_reduce.h"
#include "merge_device.h"
#include "ordered_device.h"
#include "sample_device.h"
#include "volume_device.h"
#include "align_solver.h"

namespace itm {

constexpr float kAlignPointLimit = 262136.0f;      // ITM_QUERY_INVALID's rule (query.hip: kPointLimit)

// ---- band samples ------------------------------------------------------------------------------------------------------------------------

struct BandParams {
  int minWeight, stride;
  float maxAbsSdf, voxelSize, mu;
  long long elements;          // dense: voxels; hash: noTotalEntries * 512
  size_t numVoxels;
  int sx, sy, ox, oy, oz;      // dense size (x, y) and offset
};

// The lane's eight consecutive elements from i0 on: bit k of the result says element i0 + k is kept, out[k] is then its sample.
// Hash: the eight voxels are one x-row of the block of slot i0 >> 9 (uniform per wave).
template <class VX, bool DENSE>
__device__ inline uint32_t band_mask(const void* __restrict__ vba, const uint4* __restrict__ hash, const uint8_t* __restrict__ sel, const BandParams& p, long long i0,
                                     float4 out[8]) {
  if (i0 >= p.elements) return 0u;
  long long first;      // voxel index of element i0
  int x0, y, z;         // its global coordinates
  int count = 8;
  if constexpr (DENSE) {
    first = i0;
    x0 = (int)(i0 % p.sx) + p.ox;                      // (a row of eight may run over the end of an x-line: coordinates per element below)
    y = (int)((i0 / p.sx) % p.sy) + p.oy;
    z = (int)(i0 / ((long long)p.sx * p.sy)) + p.oz;
    if (p.elements - i0 < 8) count = (int)(p.elements - i0);
  } else {
    const int slot = (int)(i0 >> 9);
    if (sel && !sel[slot]) return 0u;
    const HashEntry e = unpack_entry(hash[slot]);
    if (e.ptr < 0 || (size_t)e.ptr * kBlockVoxels + kBlockVoxels > p.numVoxels) return 0u;
    const int v = (int)(i0 & 511);
    first = (long long)e.ptr * kBlockVoxels + v;
    x0 = e.px * 8 + (v & 7); y = e.py * 8 + ((v >> 3) & 7); z = e.pz * 8 + (v >> 6);
  }
  uint32_t mask = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k >= count) break;
    int x = x0 + k, yy = y, zz = z;
    if constexpr (DENSE) {
      const long long i = i0 + k;
      x = (int)(i % p.sx) + p.ox; yy = (int)((i / p.sx) % p.sy) + p.oy; zz = (int)(i / ((long long)p.sx * p.sy)) + p.oz;
    }
    const typename VX::Reg r = VX::load(vba, (size_t)(first + k));
    const float sdf = VX::to_float(VX::raw_sdf(r));
    const bool keep = VX::w_depth(r) >= p.minWeight && fabsf(sdf) < p.maxAbsSdf && x % p.stride == 0 && yy % p.stride == 0 && zz % p.stride == 0;
    if (keep) {
      mask |= 1u << k;
      out[k] = make_float4((float)x * p.voxelSize, (float)yy * p.voxelSize, (float)zz * p.voxelSize, sdf * p.mu);
    }
  }
  return mask;
}

template <class VX, bool DENSE>
__global__ void __launch_bounds__(256) band_count_kernel(const void* __restrict__ vba, const uint4* __restrict__ hash, const uint8_t* __restrict__ sel, BandParams p,
                                                         int32_t* __restrict__ chunkCount) {
  __shared__ int lds[4];
  float4 out[8];
  const uint32_t mask = band_mask<VX, DENSE>(vba, hash, sel, p, (long long)blockIdx.x * kSweepChunk + threadIdx.x * 8, out);
  const int sum = block_reduce_sum<4>(__popc(mask), lds);
  if (threadIdx.x == 0) chunkCount[blockIdx.x] = sum;
}

// chunkBase[c] = kept elements of the chunks before c; *total = all of them.  One workgroup.
__global__ void __launch_bounds__(1024) band_scan_kernel(const int32_t* __restrict__ chunkCount, int nChunks, int32_t* __restrict__ chunkBase, int32_t* __restrict__ total) {
  const int sum = carry_scan<16, int>(nChunks, [&](int i) { return chunkCount[i]; }, [&](int i, int prefix) { chunkBase[i] = prefix; });
  if (threadIdx.x == 0) *total = sum;
}

template <class VX, bool DENSE>
__global__ void __launch_bounds__(256) band_fill_kernel(const void* __restrict__ vba, const uint4* __restrict__ hash, const uint8_t* __restrict__ sel, BandParams p,
                                                        const int32_t* __restrict__ chunkCount, const int32_t* __restrict__ chunkBase, float4* __restrict__ samples,
                                                        int capacity) {
  __shared__ int lds[kOrderedLds];
  if (chunkCount[blockIdx.x] == 0) return;                // (uniform per workgroup)
  const int base = chunkBase[blockIdx.x];
  if (base >= capacity) return;
  float4 out[8];
  const uint32_t mask = band_mask<VX, DENSE>(vba, hash, sel, p, (long long)blockIdx.x * kSweepChunk + threadIdx.x * 8, out);
  int tot;
  int pos = base + block_exclusive_scan<4>(__popc(mask), lds, &tot);
  // (a chain of `if (mask & bit)` over out[] with constant indices: out[] stays in registers)
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (mask & (1u << k)) {
      if (pos < capacity) samples[pos] = out[k];
      ++pos;
    }
}

// ---- evaluation --------------------------------------------------------------------------------------------------------------------------

struct AlignParams {
  float R[9], t[3];            // x_dst = R x_src + t, row-major R
  float voxelSize, mu;
  float scale;                 // mu / voxelSize: sdf units per voxel -> metres per metre
  float delta;                 // Huber threshold, metres
  int n;
};

template <class VX, bool DENSE>
__global__ void __launch_bounds__(kGHThreads) align_eval_kernel(VolumeView vol, const float4* __restrict__ samples, AlignParams p, GHBlockRecord* __restrict__ hostRec,
                                                                unsigned int seq) {
  __shared__ double lds[kGHWaves][kGHValues];
  __shared__ int ldsCount[kGHWaves];
  double acc[kGHValues];
#pragma unroll
  for (int i = 0; i < kGHValues; ++i) acc[i] = 0.0;
  int valid = 0;
  BlockCache cache;
  for (int i = blockIdx.x * kGHThreads + threadIdx.x; i < p.n; i += gridDim.x * kGHThreads) {
    const float4 in = samples[i];
    const float x0 = ((p.R[0] * in.x + p.R[1] * in.y) + p.R[2] * in.z) + p.t[0];
    const float x1 = ((p.R[3] * in.x + p.R[4] * in.y) + p.R[5] * in.z) + p.t[1];
    const float x2 = ((p.R[6] * in.x + p.R[7] * in.y) + p.R[8] * in.z) + p.t[2];
    float qx = x0 / p.voxelSize, qy = x1 / p.voxelSize, qz = x2 / p.voxelSize;
    const bool inRange = (fabsf(qx) < kAlignPointLimit) && (fabsf(qy) < kAlignPointLimit) && (fabsf(qz) < kAlignPointLimit);      // false for NaN and Inf too
    if (!inRange) qx = qy = qz = 0.0f;      // nothing is read at an invalid position: the lane fetches cell 0 and drops it
    Corners<VX, DENSE> cn;
    cn.fetch(vol, qx, qy, qz, cache);
    bool ok = inRange;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && cn.present[c] && VX::to_float(cn.v[c]) != 1.0f;
    if (!ok) continue;
    const float s = cn.trilinear();
    float g[3];
    trilinear_gradient<VX>(cn.v, cn.cx, cn.cy, cn.cz, g);
    const float r = p.mu * s - in.w;
    const float n0 = g[0] * p.scale, n1 = g[1] * p.scale, n2 = g[2] * p.scale;
    float j[6];
    j[0] = n0; j[1] = n1; j[2] = n2;
    j[3] = x1 * n2 - x2 * n1;
    j[4] = x2 * n0 - x0 * n2;
    j[5] = x0 * n1 - x1 * n0;
    const float a = fabsf(r);
    const bool quadratic = a <= p.delta;
    const float w = quadratic ? 1.0f : p.delta / a;
    const float rho = quadratic ? (0.5f * r) * r : p.delta * (a - 0.5f * p.delta);
    const float wr = w * r;
    ++valid;
    acc[0] += (double)rho;
#pragma unroll
    for (int rr = 0, k = 0; rr < 6; ++rr) {
      acc[1 + rr] += (double)(wr * j[rr]);
      const float wj = w * j[rr];
#pragma unroll
      for (int c = 0; c <= rr; ++c, ++k) acc[7 + k] += (double)(wj * j[c]);
    }
  }
  double mine; int cnt;
  gh_block_reduce<3>(acc, valid, lds, ldsCount, mine, cnt);
  send_record<__HIP_MEMORY_SCOPE_SYSTEM>(hostRec + blockIdx.x, mine, cnt, seq);
}

}  // namespace itm

struct itm_aligner : itm::GHHandle {
  const float4* samples = nullptr;      // the caller's device memory
  int n = 0;
};

namespace itm {

GHHandle* gh_handle(itm_aligner* a) { return static_cast<GHHandle*>(a); }

// One pass over the handle's samples at the float pose M: cost, gradient, Hessian and the valid count.
static int align_evaluate(itm_aligner* a, const itm_scene* s, const float M[16], const itm_align_config& cfg, itm_align_eval* out, hipStream_t st) {
  memset(out, 0, sizeof *out);
  if (a->n <= 0 || !a->samples) return ITM_OK;
  { const int rc = a->ready([&] { a->ch.release(); }); if (rc) return rc; }
  AlignParams p;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) p.R[3 * r + c] = M[4 * c + r];
    p.t[r] = M[12 + r];
  }
  p.voxelSize = s->prm.voxelSize; p.mu = s->prm.mu;
  p.scale = s->prm.mu / s->prm.voxelSize;
  p.delta = cfg.huberDelta;
  p.n = a->n;
  const int groups = std::min(kGHGroups, (a->n + kGHThreads - 1) / kGHThreads);
  const VolumeView vol = make_volume(s);
  double sums[kGHValues];
  int valid = 0;
  const int rc = a->evaluate((size_t)groups, st, [&](GHBlockRecord* rec, unsigned int seq) {
    return dispatch_volume(s, [&](auto vx, auto dense) {
      align_eval_kernel<decltype(vx), dense.value><<<groups, kGHThreads, 0, st>>>(vol, a->samples, p, rec, seq);
      return ITM_OK;
    });
  }, sums, &valid);
  if (rc) return rc;
  out->f = (float)sums[0];
  out->noValid = valid;
  unpack_gh(sums, 6, 6, 1.0f, out->nabla, out->hessian);
  return ITM_OK;
}

static int align_check(const float M[16], const itm_align_config* cfg, const char* what) {
  if (!M || !cfg) return set_error(ITM_ERR_INVALID, std::string(what) + ": null argument");
  const char* why = align_refusal(M, *cfg);
  return why ? set_error(ITM_ERR_INVALID, std::string(what) + ": " + why) : ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_align_default_config(float voxelSize, float mu, itm_align_config* cfg) {
  if (!cfg) return set_error(ITM_ERR_INVALID, "align default config: null argument");
  if (!std::isfinite(voxelSize) || !(voxelSize > 0.0f) || !std::isfinite(mu) || !(mu > 0.0f))
    return set_error(ITM_ERR_INVALID, "align default config: voxelSize and mu are positive finite numbers");
  cfg->minWeight = 1; cfg->maxAbsSdf = 1.0f; cfg->stride = 1;
  cfg->huberDelta = mu / 4.0f;
  cfg->minStep = 1e-5f;
  cfg->maxEvaluations = 60; cfg->minValid = 100;
  cfg->minConditioning = 1e-3f;
  return ITM_OK;
}

int itm_align_step(const itm_align_eval* eval, double lambda, float step[6]) {
  if (!eval || !step) return set_error(ITM_ERR_INVALID, "align step: null argument");
  double d[6];
  align_step(*eval, lambda, d);
  for (int i = 0; i < 6; ++i) step[i] = (float)d[i];
  return ITM_OK;
}

int itm_align_apply_step(const float pose[16], const float step[6], float out[16]) {
  if (!pose || !step || !out) return set_error(ITM_ERR_INVALID, "align apply step: null argument");
  double d[6];
  for (int i = 0; i < 6; ++i) d[i] = (double)step[i];
  se3::to_matrix(align_apply(se3::from_matrix(pose), d), out);
  return ITM_OK;
}

int itm_scene_band_samples(const itm_scene* src, const int32_t* srcSlots_dev, int n, const itm_align_config* cfg, float* samples_dev, int32_t capacity,
                           int32_t* count_out, itm_stream stream) {
  if (!src || !cfg || !count_out) return set_error(ITM_ERR_INVALID, "band samples: null argument");
  if (!(cfg->maxAbsSdf > 0.0f) || !(cfg->maxAbsSdf <= 1.0f)) return set_error(ITM_ERR_INVALID, "band samples: maxAbsSdf is in (0, 1]");
  if (cfg->stride < 1) return set_error(ITM_ERR_INVALID, "band samples: stride is at least 1");
  if (capacity < 0 || (capacity > 0 && !samples_dev)) return set_error(ITM_ERR_INVALID, "band samples: a capacity without a buffer");
  if (((uintptr_t)samples_dev & 15u) != 0) return set_error(ITM_ERR_INVALID, "band samples: samples_dev must be 16-byte aligned");
  const bool hash = src->cfg.indexType == ITM_INDEX_HASH;
  { const int rc = check_slot_list(hash, srcSlots_dev, n, "band samples", "a dense scene"); if (rc) return rc; }
  { const int rc = enter_scene(src, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  BandParams p;
  p.minWeight = cfg->minWeight; p.stride = cfg->stride; p.maxAbsSdf = cfg->maxAbsSdf;
  p.voxelSize = src->prm.voxelSize; p.mu = src->prm.mu;
  p.numVoxels = src->numVoxels;
  p.sx = src->cfg.denseSize[0]; p.sy = src->cfg.denseSize[1];
  p.ox = src->cfg.denseOffset[0]; p.oy = src->cfg.denseOffset[1]; p.oz = src->cfg.denseOffset[2];
  p.elements = hash ? (long long)src->noTotalEntries * kBlockVoxels : (long long)src->numVoxels;
  const int nChunks = (int)((p.elements + kSweepChunk - 1) / kSweepChunk);
  *count_out = 0;
  if (nChunks == 0) return ITM_OK;
  // scratch of the call (scene_ops.h: BandArena; src is const here, so nothing is kept with it)
  const BandArena a(kMsCount, (size_t)nChunks, hash && srcSlots_dev ? (size_t)src->noTotalEntries : 0);
  DeviceBuffer<void> scratch;
  ITM_HIP(scratch.alloc(a.L.bytes()));
  void* base = scratch.get();
  int32_t* dTotal = a.total.at(base); int32_t* chunkCount = a.chunkCount.at(base); int32_t* chunkBase = a.chunkBase.at(base);
  uint8_t* sel = hash && srcSlots_dev ? a.sel.at(base) : nullptr;
  if (sel) {
    MergePlacement tallies{a.stats.at(base), st};
    ITM_HIP(hipMemsetAsync(tallies.dStats, 0, kMsCount * 4, st));
    if (const int rc = select_slots(srcSlots_dev, n, src->noTotalEntries, sel, tallies, "band samples")) return rc;
  }
  const int rc = dispatch_volume(src, [&](auto vx, auto dense) {
    using VX = decltype(vx);
    band_count_kernel<VX, dense.value><<<nChunks, 256, 0, st>>>(src->vba, src->hash, sel, p, chunkCount);
    band_scan_kernel<<<1, 1024, 0, st>>>(chunkCount, nChunks, chunkBase, dTotal);
    if (capacity > 0) band_fill_kernel<VX, dense.value><<<nChunks, 256, 0, st>>>(src->vba, src->hash, sel, p, chunkCount, chunkBase, (float4*)samples_dev, capacity);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  int32_t total = 0;
  ITM_HIP(hipMemcpyAsync(&total, dTotal, 4, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  *count_out = total;
  return ITM_OK;
}

int itm_aligner_create(itm_aligner** out) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  *out = new (std::nothrow) itm_aligner();
  return *out ? ITM_OK : set_error(ITM_ERR_DEVICE, "out of host memory");
}

int itm_aligner_destroy(itm_aligner* a) {
  if (!a) return ITM_OK;
  { std::lock_guard<std::mutex> g(a->mu); a->ch.release(); }
  delete a;
  return ITM_OK;
}

int itm_aligner_set_samples(itm_aligner* a, const float* samples_dev, int32_t n, itm_stream) {
  if (!a) return set_error(ITM_ERR_INVALID, "aligner: null handle");
  if (n < 0 || (n > 0 && !samples_dev)) return set_error(ITM_ERR_INVALID, "aligner: a sample count without samples");
  if (((uintptr_t)samples_dev & 15u) != 0) return set_error(ITM_ERR_INVALID, "aligner: samples_dev must be 16-byte aligned");
  std::lock_guard<std::mutex> g(a->mu);
  a->samples = n > 0 ? (const float4*)samples_dev : nullptr;
  a->n = n;
  return ITM_OK;
}

int itm_aligner_evaluate(itm_aligner* a, const itm_scene* dst, const float dstFromSrc[16], const itm_align_config* cfg, itm_align_eval* out, itm_stream stream) {
  { const int rc = align_check(dstFromSrc, cfg, "aligner evaluate"); if (rc) return rc; }
  if (!a || !dst || !out) return set_error(ITM_ERR_INVALID, "aligner evaluate: null argument");
  { const int rc = enter_scene(dst, nullptr); if (rc) return rc; }
  std::lock_guard<std::mutex> g(a->mu);
  return align_evaluate(a, dst, dstFromSrc, *cfg, out, as_stream(stream));
}

int itm_aligner_align(itm_aligner* a, const itm_scene* dst, const float dstFromSrc_in[16], const itm_align_config* cfg, float dstFromSrc_out[16], itm_align_result* res,
                      itm_stream stream) {
  { const int rc = align_check(dstFromSrc_in, cfg, "aligner align"); if (rc) return rc; }
  if (!a || !dstFromSrc_out) return set_error(ITM_ERR_INVALID, "aligner align: null argument");
  std::lock_guard<std::mutex> g(a->mu);
  if (a->n <= 0) return set_error(ITM_ERR_INVALID, "aligner align: no samples set");
  if (!dst) return set_error(ITM_ERR_INVALID, "aligner align: null scene");
  { const int rc = enter_scene(dst, nullptr); if (rc) return rc; }
  const hipStream_t st = as_stream(stream);
  float out[16];
  itm_align_result r;
  const int rc = align_run(dstFromSrc_in, *cfg, [&](const float M[16], itm_align_eval& e) { return align_evaluate(a, dst, M, *cfg, &e, st); }, out, &r);
  if (rc) return rc;
  memcpy(dstFromSrc_out, out, sizeof out);
  if (res) *res = r;
  return ITM_OK;
}

}  // extern "C"
