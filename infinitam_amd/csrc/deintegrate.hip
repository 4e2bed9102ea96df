// deintegrate.hip -- itm_deintegrate_from_scene: one fused depth frame taken back out of the TSDF (include/itm_hip.h, "frame
// de-integration"; DESIGN.md "Frame de-integration").
//
// No reference engine removes an observation; the operation is IntegrateIntoScene (DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp
// :47-114 hash, :319-369 dense) with computeUpdatedVoxelDepthInfo / ColorInfo run backwards.  The projection, the depth pixel, eta and the
// exits are fuse_device.h's, shared with the integration; the inverse averages (unfuse_average, unfuse_colour) stand beside their
// counterparts there.
//
// MI355X design: the work split of integrate.hip -- one wave per (block, group of z-slices), persistent workgroups striding the
// device-resident visible list, nothing read back; an item's voxel runs are requested before the projection, its depth gathers are issued
// together, the first wait for the voxels stands in front of the update.  It reads and writes the bytes the integration does, so the
// integration's time is the yardstick (profiles/deintegrate_notes.md).  What the update adds per voxel is the three-way case on the old
// weight and the clamp; the statistics are ballots added up in scalar registers, one atomic per counter and wave at the wave's end
// (to striped copies of the counters, see kDsStripes), and a launch without `stats` carries none of that code.
#include <cstring>

#include "fuse_device.h"
#include "wave_utils.h"

namespace itm {

#ifndef ITM_MIRROR_FLOAT_TYPES
#define ITM_MIRROR_FLOAT_TYPES 0     // (as integrate.hip: the same switch decides whether a float scene's mirror is written)
#endif

// the statistics in device memory: itm_deintegrate_stats word for word
enum { kDsBlocks, kDsVisited, kDsTouched, kDsReset, kDsUnobserved, kDsSaturated, kDsClamped, kDsColoured, kDsColourReset, kDsCount = 16 };
static_assert(sizeof(itm_deintegrate_stats) == kDsCount * 4, "itm_deintegrate_stats layout");

// Sixteen thousand waves (BASELINE configs[1]; four times as many on configs[4]) adding to the same nine words queue up on them: measured,
// 333 us instead of 16 for the launch of configs[1], 2.25 ms instead of 0.13 on configs[4].  The waves therefore add to kDsStripes copies
// of the words, a wave to the copy of its number (64 bytes each, two to a cache line); one small workgroup adds the copies up.
constexpr int kDsStripes = 256;

// A wave's counts.  add(): from wave-uniform control flow, one ballot per counter; flush(): one atomic per counter that is not zero.
struct UnfuseTally {
  int n[kDsCount] = {};
  __device__ void add(uint32_t what) {
    const uint32_t bit[7] = {kUnfuseTouched, kUnfuseReset, kUnfuseUnobserved, kUnfuseSaturated, kUnfuseClamped, kUnfuseColoured, kUnfuseColourReset};
#pragma unroll
    for (int k = 0; k < 7; ++k) n[kDsTouched + k] += __popcll(__ballot((what & bit[k]) != 0u));
  }
  __device__ void flush(int32_t* __restrict__ stripes) const {
    if ((threadIdx.x & 63) != 0) return;
    const unsigned wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t* __restrict__ stats = stripes + (size_t)(wave % kDsStripes) * kDsCount;
#pragma unroll
    for (int k = 0; k <= kDsColourReset; ++k)
      if (n[k]) atomicAdd(&stats[k], n[k]);
  }
};

// stripes[kDsStripes][kDsCount] -> the kDsCount words behind them.  One workgroup of kDsStripes lanes.
__global__ void __launch_bounds__(kDsStripes) deintegrate_tally_kernel(int32_t* __restrict__ stripes) {
  __shared__ int lds[kDsStripes / kWave];
  for (int k = 0; k <= kDsColourReset; ++k) {
    const int total = block_reduce_sum<kDsStripes / kWave>(stripes[(size_t)threadIdx.x * kDsCount + k], lds);
    if (threadIdx.x == 0) stripes[(size_t)kDsStripes * kDsCount + k] = total;
  }
}

// The items of the integration (integrate.hip, slices_of / load_item): 4 z-slices of a block per wave, the whole block for the 4-byte voxel.
template <class VX> __host__ __device__ constexpr int unfuse_slices_of() { return VX::kBytes == 4 ? 8 : 4; }

template <class VX>
__device__ inline void unfuse_load_item(const HashEntry& he, int z0, int lane, const void* __restrict__ vba, typename VX::Reg r[unfuse_slices_of<VX>()]) {
  constexpr int kSlices = unfuse_slices_of<VX>();
  const size_t vi = (size_t)(he.ptr < 0 ? 0 : he.ptr) * kBlockVoxels + (size_t)z0 * 64 + lane;      // block 0 is always there
#pragma unroll
  for (int k = 0; k < kSlices; ++k) r[k] = VX::load(vba, vi + 64 * k);
}

// r: the item's voxels (already requested).  The stages are integrate_item's; what differs is stage 3.
template <class VX, bool STATS>
__device__ inline void deintegrate_item(const HashEntry& he, int z0, int lane, typename VX::Reg r[unfuse_slices_of<VX>()], void* __restrict__ vba, void* __restrict__ sdfMirror,
                                        const float* __restrict__ depth, const uchar4* __restrict__ rgb, const FuseParams& p, int keepSaturated, UnfuseTally& tally) {
  constexpr int kSlices = unfuse_slices_of<VX>();
  const bool present = he.ptr >= 0;
  const int x = lane & 7, y = lane >> 3;
  const size_t vi = (size_t)(present ? he.ptr : 0) * kBlockVoxels + (size_t)z0 * 64 + lane;
  const float mx = (float)(he.px * kBlockSide + x) * p.voxelSize;
  const float my = (float)(he.py * kBlockSide + y) * p.voxelSize;
  const AccelWriter aw{nullptr, nullptr, nullptr, sdfMirror, 0, p.org};      // (mirror-only: block_base_wave_uniform and store_sdf alone)
  size_t mbase = 0;
  bool mirror = false;
  if constexpr (VX::kShort || ITM_MIRROR_FLOAT_TYPES) {
    mirror = aw.block_base_wave_uniform<false>(he.px, he.py, he.pz, mbase);      // (one block per wave)
  }
  int pix[kSlices];
  float pcz[kSlices], mz[kSlices];
#pragma unroll
  for (int k = 0; k < kSlices; ++k) mz[k] = (float)(he.pz * kBlockSide + z0 + k) * p.voxelSize;
  // one range decision per item for the short voxel types (integrate_item has the argument)
  bool inRange = false;
  if constexpr (ITM_FAST_DIVISIONS && VX::kShort) {
    const float za = transform_point(p.M_d, mx, my, mz[0]).z, zb = transform_point(p.M_d, mx, my, mz[kSlices - 1]).z;
    const bool ok = za >= 1e-4f && za <= 1e4f && zb >= 1e-4f && zb <= 1e4f;
    inRange = present && __builtin_amdgcn_ballot_w64(ok) == __builtin_amdgcn_ballot_w64(true);
  }
  if (inRange) {
#pragma unroll
    for (int k = 0; k < kSlices; ++k) pix[k] = fuse_depth_project<false, true>(mx, my, mz[k], p, pcz[k]);
  } else {
#pragma unroll
    for (int k = 0; k < kSlices; ++k) pix[k] = present ? fuse_depth_project<false>(mx, my, mz[k], p, pcz[k]) : -2;     // -2: no block
  }
  float dm[kSlices];
#pragma unroll
  for (int k = 0; k < kSlices; ++k) dm[k] = depth[pix[k] >= 0 ? pix[k] : 0];
  // every gather is issued here, before the first look at a voxel
#pragma unroll
  for (int k = 0; k < kSlices; ++k) asm volatile("" : "+v"(dm[k]));
#pragma unroll
  for (int k = 0; k < kSlices; ++k) {
    uint32_t what = 0u;
    if (pix[k] != -2) {
      if (unfuse_kept<VX>(r[k], p, keepSaturated)) {      // (skipped altogether, colour included)
        if (pix[k] >= 0 && !(dm[k] <= 0.0f) && !(dm[k] - pcz[k] < -p.mu)) what = kUnfuseSaturated;
      } else {
        const float eta = (pix[k] >= 0) ? unfuse_depth_update<VX>(r[k], dm[k], pcz[k], p, what) : -1.0f;
        if constexpr (VX::kColor) {
          if (in_colour_band(eta, p)) what |= unfuse_colour<VX>(r[k], mx, my, mz[k], rgb, p, keepSaturated);
        }
        if (what & (kUnfuseTouched | kUnfuseColoured)) {
          VX::store(vba, vi + 64 * k, r[k]);
          if (mirror) aw.store_sdf<VX>(mbase, mirror_block_voxel((uint32_t)x, (uint32_t)y, (uint32_t)(z0 + k)), VX::raw_sdf(r[k]));
        }
      }
    }
    if constexpr (STATS) tally.add(what);
  }
  if constexpr (STATS) {
    if (present) { tally.n[kDsVisited] += kSlices * 64; tally.n[kDsBlocks] += (z0 == 0) ? 1 : 0; }
  }
}

// integrate_hash_body's loop: the id of the wave's first item is fetched beside the list's state, the entry one item ahead and the id two
// items ahead are requested at the top of an item and looked at behind it.
template <class VX, bool STATS>
__global__ void __launch_bounds__(512) deintegrate_hash_kernel(const int32_t* __restrict__ visibleIds, const RenderCounters* __restrict__ rc,
                                                               const uint4* __restrict__ hash, void* __restrict__ vba, void* __restrict__ sdfMirror,
                                                               const float* __restrict__ depth, const uchar4* __restrict__ rgb, FuseParams p,
                                                               int keepSaturated, int32_t* __restrict__ stats) {
  constexpr int kSlices = unfuse_slices_of<VX>();
  constexpr int kItemsPerBlock = kBlockSide / kSlices;
  const int lane = threadIdx.x & 63;
  const int waves = (int)gridDim.x * (int)(blockDim.x >> 6);
  int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6));
  const int idsLast = p.idsCap - 1;
  const int at0 = i / kItemsPerBlock;
  int idCur = visibleIds[at0 < idsLast ? at0 : idsLast];
  int invalid = rc->listInvalid, nv = rc->noVisibleEntries;
  asm volatile("" : "+s"(idCur), "+s"(invalid), "+s"(nv));
  if (invalid) return;                                // the list is not the frame's: the integration fused nothing through it either
  const int nItems = nv * kItemsPerBlock;
  if (i >= nItems) return;
  int nxt = i + waves;
  int idNext = visibleIds[(nxt < nItems ? nxt : nItems - 1) / kItemsPerBlock];
  HashEntry cur = unpack_entry(hash[idCur]);
  typename VX::Reg r[kSlices];
  unfuse_load_item<VX>(cur, (i % kItemsPerBlock) * kSlices, lane, vba, r);
  UnfuseTally tally;
  for (;;) {
    const bool more = nxt < nItems;
    uint4 rawAhead = hash[idNext];
    const int after = nxt + waves;
    int idAfter = visibleIds[(after < nItems ? after : nItems - 1) / kItemsPerBlock];
    deintegrate_item<VX, STATS>(cur, (i % kItemsPerBlock) * kSlices, lane, r, vba, sdfMirror, depth, rgb, p, keepSaturated, tally);
    asm volatile("" : "+s"(rawAhead.x), "+s"(rawAhead.y), "+s"(rawAhead.z), "+s"(rawAhead.w), "+s"(idAfter));
    if (!more) break;
    cur = unpack_entry(rawAhead);
    unfuse_load_item<VX>(cur, (nxt % kItemsPerBlock) * kSlices, lane, vba, r);
    i = nxt; nxt = after; idNext = idAfter;
  }
  if constexpr (STATS) tally.flush(stats);
}

// Dense volume: one voxel per lane, x fastest, in the shape of integrate_dense_kernel.  Every lane of a wave makes the same number of
// trips (the bound is the wave's first voxel), so the ballots of the tally stand in uniform control flow.
template <class VX, bool STATS>
__global__ void __launch_bounds__(256) deintegrate_dense_kernel(void* __restrict__ vba, const float* __restrict__ depth, const uchar4* __restrict__ rgb, FuseParams p,
                                                                int sx, int sy, int sz, int ox, int oy, int oz, int keepSaturated, int32_t* __restrict__ stats) {
  const size_t n = (size_t)sx * sy * sz;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  UnfuseTally tally;
  for (size_t first = (size_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); first < n; first += stride) {
    const size_t loc = first + lane;
    uint32_t what = 0u;
    if (loc < n) {
      const int z = (int)(loc / ((size_t)sx * sy));
      const int rem = (int)(loc - (size_t)z * sx * sy);
      const int y = rem / sx;
      const int x = rem - y * sx;
      typename VX::Reg r = VX::load(vba, loc);
      const float mx = (float)(x + ox) * p.voxelSize, my = (float)(y + oy) * p.voxelSize, mz = (float)(z + oz) * p.voxelSize;
      what = unfuse_voxel<VX>(r, mx, my, mz, depth, rgb, p, keepSaturated);
      if (what & (kUnfuseTouched | kUnfuseColoured)) VX::store(vba, loc, r);
    }
    if constexpr (STATS) {
      tally.add(what);
      tally.n[kDsVisited] += __popcll(__ballot(loc < n));
    }
  }
  if constexpr (STATS) tally.flush(stats);
}

// FuseParams of a view, as launch_integrate (integrate.hip) fills them
static void fuse_params_of(const itm_scene* s, const itm_view* v, const itm_render_state* rs, FuseParams& p) {
  memcpy(p.M_d.m, v->M_d, 64);
  matmul4(v->rgb_to_depth_inv, v->M_d, p.M_rgb.m);
  p.fx = v->intr_d[0]; p.fy = v->intr_d[1]; p.cx = v->intr_d[2]; p.cy = v->intr_d[3];
  p.fxc = v->intr_rgb[0]; p.fyc = v->intr_rgb[1]; p.cxc = v->intr_rgb[2]; p.cyc = v->intr_rgb[3];
  p.mu = s->prm.mu; p.voxelSize = s->prm.voxelSize; p.maxW = s->prm.maxW;
  p.rcpMu = 1.0f / p.mu;
  uint32_t bits; memcpy(&bits, &p.mu, 4);
  p.muFast = ((bits & 0x7fffffu) != 0x7fffffu) && p.mu >= 1e-6f && p.mu <= 1e6f;
  p.W = v->w; p.H = v->h; p.Wc = v->w_rgb; p.Hc = v->h_rgb;
  p.stopAtMax = s->prm.stopIntegratingAtMaxW;      // (not consulted: keepSaturated travels beside the parameters)
  p.org = s->org;
  p.idsCap = rs->capIds > 0 ? rs->capIds : 1;
}

static int launch_deintegrate(itm_scene* s, const itm_view* v, itm_render_state* rs, int keepSaturated, int32_t* dStats, hipStream_t st) {
  FuseParams p;
  fuse_params_of(s, v, rs, p);
  const uchar4* rgb = (const uchar4*)v->rgb;
  const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
    using VX = decltype(vx);
    if (s->cfg.indexType == ITM_INDEX_HASH) {
      // the integration's stand-alone launch: 256-lane workgroups, twice the 2 048 / 8 192 of the 512-lane form (integrate.hip has the measurements)
      const int grid = ((size_t)rs->w * rs->h > (size_t)640 * 480 ? 8192 : 2048) * 2;
      if (dStats) deintegrate_hash_kernel<VX, true><<<grid, 256, 0, st>>>(rs->visibleIds, rs->counters, s->hash, s->vba, s->sdfMirror, v->depth, rgb, p, keepSaturated, dStats);
      else deintegrate_hash_kernel<VX, false><<<grid, 256, 0, st>>>(rs->visibleIds, rs->counters, s->hash, s->vba, s->sdfMirror, v->depth, rgb, p, keepSaturated, nullptr);
    } else {
      const int* sz = s->cfg.denseSize; const int* of = s->cfg.denseOffset;
      if (dStats) deintegrate_dense_kernel<VX, true><<<256 * 32, 256, 0, st>>>(s->vba, v->depth, rgb, p, sz[0], sz[1], sz[2], of[0], of[1], of[2], keepSaturated, dStats);
      else deintegrate_dense_kernel<VX, false><<<256 * 32, 256, 0, st>>>(s->vba, v->depth, rgb, p, sz[0], sz[1], sz[2], of[0], of[1], of[2], keepSaturated, nullptr);
    }
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  if (dStats) {
    deintegrate_tally_kernel<<<1, kDsStripes, 0, st>>>(dStats);
    ITM_LAUNCH_CHECK();
  }
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" int itm_deintegrate_from_scene(itm_scene* s, const itm_view* v, itm_render_state* rs, const itm_deintegrate_config* cfg, itm_deintegrate_stats* stats,
                                          itm_stream stream) {
  if (!s || !v || !rs) return set_error(ITM_ERR_INVALID, "deintegrate: null argument");
  if (!v->depth) return set_error(ITM_ERR_INVALID, "deintegrate: null depth image");
  if (rs->scene != s) return set_error(ITM_ERR_INVALID, "deintegrate: render state belongs to another scene");
  { const int rc = validate_integrate(s, v); if (rc) return rc; }
  if (cfg && cfg->keepSaturated != 0 && cfg->keepSaturated != 1) return set_error(ITM_ERR_INVALID, "deintegrate: keepSaturated is neither 0 nor 1");
  { const int rc = enter_scene(s, rs); if (rc) return rc; }      // a frame recorded for the fused launch goes first
  const int keepSaturated = cfg ? cfg->keepSaturated : (s->prm.stopIntegratingAtMaxW ? 1 : 0);
  hipStream_t st = as_stream(stream);
  int32_t* dStats = nullptr;
  if (stats) {
    ITM_HIP(s->deintegrateStats.reserve((size_t)(kDsStripes + 1) * kDsCount));      // the stripes, then their sums
    dStats = s->deintegrateStats.get();
    ITM_HIP(hipMemsetAsync(dStats, 0, (size_t)(kDsStripes + 1) * kDsCount * sizeof(int32_t), st));
  }
  { const int rc = launch_deintegrate(s, v, rs, keepSaturated, dStats, st); if (rc) return rc; }
  if (stats) {
    ITM_HIP(hipMemcpyAsync(stats, dStats + (size_t)kDsStripes * kDsCount, sizeof *stats, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
  }
  return ITM_OK;
}
