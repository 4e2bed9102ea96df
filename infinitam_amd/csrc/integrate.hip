// integrate.hip -- IntegrateIntoScene: the launch, and the hash engine.
//
// Reference behaviour:
//   IntegrateIntoScene (hash)   DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:47-114
// The per-voxel arithmetic both engines share is in fuse_device.h, the dense engine in integrate_dense.hip.
//
// MI355X design: the hash kernel gives (block, 4 z-slices) to ONE WAVE -- four contiguous 64-voxel runs in flight together, then
// four depth gathers together -- with 2 048 workgroups of 8 waves striding over the device-resident visible list, so no count is
// read back; voxels of the short types are mirrored into the position-addressed sdf copy the ray caster reads (accel_device.h).
#include <cstring>

#include "fuse_device.h"
#include "range_device.h"

namespace itm {

#ifndef ITM_EXP_FUSED_STAMPS
#define ITM_EXP_FUSED_STAMPS 0
#endif
#ifndef ITM_MIRROR_FLOAT_TYPES
#define ITM_MIRROR_FLOAT_TYPES 0     // (scene.hip decides whether a float scene gets a mirror; the same switch must be given to both files)
#endif

// Work item = kSlices consecutive z-slices of one visible block, done by ONE WAVE: lane <-> (x, y), one 64-voxel run per slice.
// The persistent waves stride over the items (item i = block i / (8 / kSlices), slice group i % (8 / kSlices)), so the waves of a
// workgroup sit on the same block or its list neighbours, and no wave ever waits for another.
//
// Why a wave and not a workgroup per block (rounds 1 and 2 until here: 512 lanes on one block, one voxel per lane): the counters
// (profiles/r2_integrate_counters.md) show the hash kernels at 43-46 % VALU utilisation with waves waiting 62-80 % of their time:
// every block costs a chain of dependent round trips -- list position -> hash entry -> voxels -> depth pixel (-> colour pixels) ->
// store -- and a wave had just 64 voxels (256-768 B) in flight along it.  32 waves x 768 B per CU over ~2 us of loaded latency is
// 3.1 TB/s for the whole chip, which is exactly what BASELINE configs[4] measured.  Here a wave has kSlices runs in flight at once
// (their loads are issued together, then the projections, then the depth gathers together), the entry of its NEXT item is
// requested before it starts on the current one, and the x / y partial sums of the projection are shared by the slices.
// (Two x-neighbours per lane with packed fp32 arithmetic -- v_pk_mul / add / fma_f32, bit-exact -- was built and measured first:
// -8 % VALU instructions, but +5 % time; the kernels are not VALU bound.)
// Slices per item: 4 (1 / 2 / 8: 243 / 211 / 195 us against 186 on BASELINE configs[4] when it was chosen).  ITMVoxel_s (4 bytes, 36 registers)
// takes the whole block per item -- eight runs in flight per wave; end of round 4, BASELINE configs[1], integration + projection launch:
// 2 slices 22.5-23.0 us, 4: 20.4-20.5, 8: 19.2-19.5; the 12-byte ITMVoxel_f_rgb loses with 8 (configs[4]: 178 -> 196 us, registers).
// (Also measured and not kept, profiles/r4_integrate_notes.md: a whole block per wave with 16 bytes per lane, for all four voxel types --
// configs[1] 19.9 -> 20.8-22.1 us, configs[4] 180 -> 264; the next item's voxel runs requested behind the depth gathers -- configs[4]
// 189 -> 198 us, the second register set costs a wave of occupancy; non-temporal stores of the voxels or of the mirror values: +-0 / +2 us
// on the ray cast that follows.)
constexpr int kIntegrateSlices = 4, kIntegrateSlicesShort = 8;
template <class VX> __host__ __device__ constexpr int slices_of() { return VX::kBytes == 4 ? kIntegrateSlicesShort : kIntegrateSlices; }

template <class VX>
__device__ inline void load_item(const HashEntry& he, int z0, int lane, const void* __restrict__ vba, typename VX::Reg r[slices_of<VX>()]) {
  constexpr int kSlices = slices_of<VX>();
  const size_t vi = (size_t)(he.ptr < 0 ? 0 : he.ptr) * kBlockVoxels + (size_t)z0 * 64 + lane;      // block 0 is always there
#pragma unroll
  for (int k = 0; k < kSlices; ++k) r[k] = VX::load(vba, vi + 64 * k);
}

// r: the item's voxels (already requested)
template <class VX>
__device__ inline void integrate_item(const HashEntry& he, int z0, int lane, typename VX::Reg r[slices_of<VX>()], void* __restrict__ vba, void* __restrict__ sdfMirror,
                                      const float* __restrict__ depth, const uchar4* __restrict__ rgb, const FuseParams& p) {
  constexpr int kSlices = slices_of<VX>();
  const bool present = he.ptr >= 0;
  const int x = lane & 7, y = lane >> 3;
  const size_t vi = (size_t)(present ? he.ptr : 0) * kBlockVoxels + (size_t)z0 * 64 + lane;
  const float mx = (float)(he.px * kBlockSide + x) * p.voxelSize;
  const float my = (float)(he.py * kBlockSide + y) * p.voxelSize;
  // (a MIRROR-ONLY writer: the integration stores mirror values and nothing else, and the mirror's origin travels in FuseParams.  Only
  // block_base_wave_uniform and store_sdf may be called on it -- no bitmap, no directories, and mirrorFloat is not consulted by either)
  const AccelWriter aw{nullptr, nullptr, nullptr, sdfMirror, 0, p.org};
  size_t mbase = 0;
  bool mirror = false;
  // (the block's page was mapped when the block was allocated; the table entry is requested here, beside the voxels, and used at the end.
  // The float voxel types carry no mirror unless built with ITM_MIRROR_FLOAT_TYPES: their kernels do not carry its code either -- two
  // registers more and ITMVoxel_f_rgb drops from six waves per SIMD to five, 180 -> 203 us on BASELINE configs[4])
  if constexpr (VX::kShort || ITM_MIRROR_FLOAT_TYPES) {
    mirror = aw.block_base_wave_uniform<false>(he.px, he.py, he.pz, mbase);      // (one block per wave)
  }
  // stage 1: project every slice's voxel; stage 2: all depth pixels together; stage 3: update (+ colour), store what changed.
  // Stages 1 and 2 do not look at the voxels: the item's runs (requested by the caller) are still on their way while the wave projects
  // and gathers, and the first wait for them stands in front of stage 3.  (Until round 6 the stopIntegratingAtMaxW test -- which reads
  // the voxel's weight -- stood in front of the projection: the compiler's s_waitcnt for run k preceded the projection of slice k, so a
  // wave idled through the voxels' round trip and then through the depth pixels' instead of through the longer of the two.)
  int pix[kSlices];
  float pcz[kSlices], mz[kSlices];
#pragma unroll
  for (int k = 0; k < kSlices; ++k) mz[k] = (float)(he.pz * kBlockSide + z0 + k) * p.voxelSize;
  // ONE range decision per item instead of one per voxel (short voxel types; the second copy of the projection would cost ITMVoxel_f_rgb
  // three registers).  fuse_depth_project takes its short, division-free form for pc.z in [1e-4, 1e4] and leaves at pc.z <= 0.
  // pc.z = ((m2 mx + m6 my) + m10 mz) + m14 is evaluated in float without contraction; along a lane's column only mz changes,
  // mz[k] = (float)(integer) * voxelSize is monotone in k, and a rounded product and a rounded sum are monotone in each operand: a lane's
  // pc.z values are monotone in k, so all of them lie between the first slice's and the last's.  (Should an intermediate overflow, an end
  // value is infinite or NaN and fails the test.)  Both ends inside the range for EVERY lane -- one ballot -- therefore shows exactly, with
  // no margin to argue about, that every voxel of the item takes the short form and none the pc.z <= 0 exit; the projection compiled for
  // that case has neither the tests nor the IEEE divisions in it.  Any other item runs the per-voxel code
  // (tests/test_integrate_uniform_paths.py restates the decision in float32 and checks it against every voxel of blocks at the bounds).
  // Measured on BASELINE configs[1]: -6 % vector, -14 % scalar instructions per launch (profiles/integrate_uniform_notes.md).
  bool inRange = false;
  if constexpr (ITM_FAST_DIVISIONS && VX::kShort) {
    const float za = transform_point(p.M_d, mx, my, mz[0]).z, zb = transform_point(p.M_d, mx, my, mz[kSlices - 1]).z;      // (the values the projections below compute again)
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
  // every gather is issued HERE, before the first look at a voxel (left alone the compiler sinks the gather of a slice into that slice's
  // conditional update, behind the wait for the slice's voxels)
#pragma unroll
  for (int k = 0; k < kSlices; ++k) asm volatile("" : "+v"(dm[k]));
#pragma unroll
  for (int k = 0; k < kSlices; ++k) {
    if (pix[k] == -2 || (p.stopAtMax && VX::w_depth(r[k]) == p.maxW)) continue;      // (a saturated voxel is skipped altogether, colour included)
    bool touched = false;
    const float eta = (pix[k] >= 0) ? fuse_depth_update<VX>(r[k], dm[k], pcz[k], p, touched) : -1.0f;
    if constexpr (VX::kColor) {
      if (in_colour_band(eta, p)) {
        fuse_colour<VX>(r[k], mx, my, mz[k], rgb, p);
        touched = true;
      }
    }
    if (touched) {
      VX::store(vba, vi + 64 * k, r[k]);
      if (mirror) aw.store_sdf<VX>(mbase, mirror_block_voxel((uint32_t)x, (uint32_t)y, (uint32_t)(z0 + k)), VX::raw_sdf(r[k]));
    }
  }
}

template <class VX>
__device__ inline void integrate_hash_body(int wgIdx, int wgCount, const int32_t* __restrict__ visibleIds, RenderCounters* __restrict__ rc,
                                           const uint4* __restrict__ hash, void* __restrict__ vba, void* __restrict__ sdfMirror,
                                           const float* __restrict__ depth, const uchar4* __restrict__ rgb, const FuseParams& p) {
  constexpr int kSlices = slices_of<VX>();
  constexpr int kItemsPerBlock = kBlockSide / kSlices;
  const int lane = threadIdx.x & 63;
  const int waves = wgCount * (int)(blockDim.x >> 6);
  int i = __builtin_amdgcn_readfirstlane(wgIdx * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6));
  // What a wave needs before it can ask for its first voxels is a chain of scalar round trips to memory the previous launch has just
  // written: the list's state, the id at the wave's position, the table entry behind the id.  The first two do not depend on each other --
  // the id is fetched speculatively (the position is clamped to the list's capacity; the value is only used once the count says it is
  // one) -- so they travel together: three round trips to the first voxel request instead of five (until round 6: listInvalid, then the
  // count, then the id, then the entry).
  const int idsLast = p.idsCap - 1;
  const int at0 = i / kItemsPerBlock;
  int idCur = visibleIds[at0 < idsLast ? at0 : idsLast];
  int invalid = rc->listInvalid, nv = rc->noVisibleEntries;
  asm volatile("" : "+s"(idCur), "+s"(invalid), "+s"(nv));      // all three requested above this line, looked at below it
  if (invalid) return;                                // the list of this frame is not the reference's: fuse nothing (alloc.hip, statusFlags bit 1)
  const int nItems = nv * kItemsPerBlock;
  if (i >= nItems) return;
  // the id of the NEXT item travels with the first entry; inside the loop the entry one item ahead and the id two items ahead are requested
  // at the top of an item and looked at behind it (positions clamped to the list's end: a wave without a next item re-reads its last)
  int nxt = i + waves;
  int idNext = visibleIds[(nxt < nItems ? nxt : nItems - 1) / kItemsPerBlock];
  HashEntry cur = unpack_entry(hash[idCur]);
  typename VX::Reg r[kSlices];
  load_item<VX>(cur, (i % kItemsPerBlock) * kSlices, lane, vba, r);
  // (the next item's VOXELS in a second register set, so that the launch could have no more waves than the device holds -- every item in
  // flight from the first microsecond -- was built and measured in round 6 on BASELINE configs[1]: 768 workgroups 21.9-22.3 us, 1 024:
  // 20.5, against 19.0-19.4 for 2 048 workgroups without it; and so was a wave that owns TWO blocks and works on them together -- sixteen
  // runs, sixteen projections, sixteen gathers, one wait, 80 registers, every block of the frame in flight from the first microsecond on
  // 768 resident workgroups: 20.5-21.0 us, the workgroups then last 9-18 us each.  A wave with two blocks takes twice as long as a wave
  // with one, whatever is prefetched or interleaved: the launch is bound by what the blocks cost to work through, not by the chain
  // (profiles/r6_notes.md).)
  for (;;) {
    const bool more = nxt < nItems;
    uint4 rawAhead = hash[idNext];
    const int after = nxt + waves;
    int idAfter = visibleIds[(after < nItems ? after : nItems - 1) / kItemsPerBlock];
    integrate_item<VX>(cur, (i % kItemsPerBlock) * kSlices, lane, r, vba, sdfMirror, depth, rgb, p);
    asm volatile("" : "+s"(rawAhead.x), "+s"(rawAhead.y), "+s"(rawAhead.z), "+s"(rawAhead.w), "+s"(idAfter));
    if (!more) break;
    cur = unpack_entry(rawAhead);
    load_item<VX>(cur, (nxt % kItemsPerBlock) * kSlices, lane, vba, r);
    i = nxt; nxt = after; idNext = idAfter;
  }
}

#ifndef ITM_INTEGRATE_BLOCK
#define ITM_INTEGRATE_BLOCK 256          // lanes per workgroup of the stand-alone launch: at 72 registers a SIMD holds 7 waves, which 8-wave workgroups cannot fill (6); measured 134.5 -> 120.9 us on BASELINE configs[4]
#endif
#ifdef ITM_INTEGRATE_WAVES_PER_EU
#define ITM_INTEGRATE_OCC __attribute__((amdgpu_waves_per_eu(ITM_INTEGRATE_WAVES_PER_EU, ITM_INTEGRATE_WAVES_PER_EU)))
#else
#define ITM_INTEGRATE_OCC
#endif
template <class VX>
__global__ void __launch_bounds__(512) ITM_INTEGRATE_OCC integrate_hash_kernel(const int32_t* __restrict__ visibleIds, RenderCounters* __restrict__ rc,
                                                             const uint4* __restrict__ hash, void* __restrict__ vba, void* __restrict__ sdfMirror,
                                                             const float* __restrict__ depth, const uchar4* __restrict__ rgb, FuseParams p) {
  integrate_hash_body<VX>(blockIdx.x, gridDim.x, visibleIds, rc, hash, vba, sdfMirror, depth, rgb, p);
}

// IntegrateIntoScene and the projection half of CreateExpectedDepths in ONE launch: both only depend on the
// visible list, integration is ALU bound on every CU while the kRangeParts projection workgroups are bound by
// LDS atomics on 32 CUs, so they overlap almost perfectly (17 + 11.5 us as two launches -> ~19 us).  The first
// kRangeParts workgroups project, the others are the persistent integration workgroups.
#if ITM_EXP_FUSED_STAMPS
// measurement build: per-workgroup start / end of the fused launch on the constant-rate global clock (100 MHz)
__device__ unsigned long long g_fusedStamps[8192 * 2];
#define ITM_FS(...) __VA_ARGS__
#else
#define ITM_FS(...)
#endif
template <class VX>
__global__ void __launch_bounds__(512) integrate_project_kernel(const int32_t* __restrict__ visibleIds, RenderCounters* __restrict__ rc,
                                                                const uint4* __restrict__ hash, void* __restrict__ vba, void* __restrict__ sdfMirror,
                                                                const float* __restrict__ depth, const uchar4* __restrict__ rgb, FuseParams p,
                                                                float2* __restrict__ range, uint4* __restrict__ projBuf, uint2* __restrict__ partials,
                                                                ProjParams pp, int RW, int RH) {
  extern __shared__ uint2 cells[];
  ITM_FS(if (threadIdx.x == 0 && blockIdx.x < 8192) g_fusedStamps[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();)
  if (blockIdx.x < kRangeParts) {
    // the few projection workgroups share their CUs with integration workgroups and would otherwise be the last to finish
    // (21.8 us fused against 15.7 us for the integration alone): let their waves win the issue arbitration
    __builtin_amdgcn_s_setprio(3);
    project_partial_body(blockIdx.x, cells, visibleIds, rc, hash, range, projBuf, partials, pp, RW, RH);
    ITM_FS(__syncthreads(); if (threadIdx.x == 0) g_fusedStamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();)
    return;
  }
  integrate_hash_body<VX>(blockIdx.x - kRangeParts, gridDim.x - kRangeParts, visibleIds, rc, hash, vba, sdfMirror, depth, rgb, p);
  ITM_FS(__syncthreads(); if (threadIdx.x == 0 && blockIdx.x < 8192) g_fusedStamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();)
}
#if ITM_EXP_FUSED_STAMPS
extern "C" int itm_debug_read_fused_stamps(unsigned long long* dst, int n) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_fusedStamps), (size_t)n * 8); }
#endif

// `fuseProjection`: also run the projection half of CreateExpectedDepths (hash scenes whose sub-sampled range image
// fits four times in LDS; the caller checked can_fuse_projection and launches range_reduce afterwards).
// what an integration of view `v` would be refused for (checked at once by the entry point that records the call, pending.hip)
int validate_integrate(const itm_scene* s, const itm_view* v) {
  const bool colour = voxel_has_colour(s->cfg.voxelType);
  if (colour && (!v->rgb || v->w_rgb <= 0 || v->h_rgb <= 0)) return set_error(ITM_ERR_INVALID, "colour voxels need an rgb image");
  return ITM_OK;
}

int launch_integrate(itm_scene* s, const itm_view* v, itm_render_state* rs, hipStream_t st, bool fuseProjection) {
  FuseParams p;
  memcpy(p.M_d.m, v->M_d, 64);
  matmul4(v->rgb_to_depth_inv, v->M_d, p.M_rgb.m);  // calib_inv * M_d (_CPU.cpp:61)
  p.fx = v->intr_d[0]; p.fy = v->intr_d[1]; p.cx = v->intr_d[2]; p.cy = v->intr_d[3];
  p.fxc = v->intr_rgb[0]; p.fyc = v->intr_rgb[1]; p.cxc = v->intr_rgb[2]; p.cyc = v->intr_rgb[3];
  p.mu = s->prm.mu; p.voxelSize = s->prm.voxelSize; p.maxW = s->prm.maxW;
  {
    // 1/mu correctly rounded (host division); the fast quotient needs a normal mu whose significand is
    // not all ones and a magnitude that keeps eta/mu far from overflow/underflow
    p.rcpMu = 1.0f / p.mu;
    uint32_t bits; memcpy(&bits, &p.mu, 4);
    p.muFast = ((bits & 0x7fffffu) != 0x7fffffu) && p.mu >= 1e-6f && p.mu <= 1e6f;
  }
  p.W = v->w; p.H = v->h; p.Wc = v->w_rgb; p.Hc = v->h_rgb;
  p.stopAtMax = s->prm.stopIntegratingAtMaxW;
  p.org = s->org;
  p.idsCap = rs->capIds > 0 ? rs->capIds : 1;
  const uchar4* rgb = (const uchar4*)v->rgb;
  { const int rc = validate_integrate(s, v); if (rc) return rc; }

  if (s->cfg.indexType == ITM_INDEX_HASH) {
    KernelTimer tk(s, ITM_TK_INTEGRATE, st);
    // 2048 workgroups of 8 waves: more waves than the chip holds at once (768-1024 workgroups), so that the dispatcher evens out what
    // the static striding does not, but few enough that most waves have work -- a workgroup without any still holds a slot for ~1 us
    // (measured, configs[4] / configs[1]: 768-1024 workgroups 189 / 21.3 us, 1536: 177 / 19.9, 2048: 175 / 20.3, 4096: 170 / 20.4,
    // where the last workgroup of configs[1] only STARTS after 15 us)
    // re-measured at the end of round 4 on the final kernels (ITMVoxel_s with a whole block per item): 640 x 480 (9.6 k visible blocks)
    // 1024: 19.5-19.8 us, 1536: 19.4-19.8, 2048: 19.0-19.5, 3072: 18.9-19.8, 8192: 18.2-19.6; 1280 x 960 colour (55.8 k blocks) 1024: 193 us,
    // 2048: 178, 3072: 174, 4096: 173-174, 6144: 172-173, 8192: 171 -- the number of visible blocks is not known on the host (nothing is read
    // back), the image size stands in for it
    const int grid = debug_value(ITM_DEBUG_INTEGRATE_WORKGROUPS) > 0 ? debug_value(ITM_DEBUG_INTEGRATE_WORKGROUPS) : ((size_t)rs->w * rs->h > (size_t)640 * 480 ? 8192 : 2048);
    ProjParams pp;
    const int RW = (rs->w + 7) / 8, RH = (rs->h + 7) / 8;
    if (fuseProjection) {
      memcpy(pp.M.m, v->M_d, 64);
      pp.fx = v->intr_d[0]; pp.fy = v->intr_d[1]; pp.cx = v->intr_d[2]; pp.cy = v->intr_d[3];
      pp.voxelSize = s->prm.voxelSize; pp.W = rs->w; pp.H = rs->h; pp.maxBlocks = s->cfg.maxRenderingBlocks;
    }
    int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      if (fuseProjection)
        integrate_project_kernel<VX><<<grid, 512, (size_t)RW * RH * sizeof(uint2), st>>>(rs->visibleIds, rs->counters, s->hash, s->vba, s->sdfMirror, v->depth, rgb, p,
                                                                                         rs->range, rs->projBuf, rs->rangePartials, pp, RW, RH);
      else integrate_hash_kernel<VX><<<grid * (512 / ITM_INTEGRATE_BLOCK), ITM_INTEGRATE_BLOCK, 0, st>>>(rs->visibleIds, rs->counters, s->hash, s->vba, s->sdfMirror, v->depth, rgb, p);
      return ITM_OK;
    });
    if (rc) return rc;
  } else {
    const int rc = launch_integrate_dense(s, v, p, st);
    if (rc) return rc;
  }
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // namespace itm

