// raycast_device.h -- the ray march shared by the visualisation kernels and the ray queries, over the voxel reads of volume_device.h.
//
// Reference behaviour restated (operation order: SURVEY.md Appendix A.6-A.8):
//   castRay                                           DeviceAgnostic/ITMVisualisationEngine.h:92-158
#pragma once

#include "volume_device.h"

#ifndef ITM_EXP_WAVE_TIMING
#define ITM_EXP_WAVE_TIMING 0  // measurement build: per-wave cycle accounting of cast_ray (tools/wave_stats.py)
#endif

namespace itm {

// ---- launch constants of the march (each swept on the final kernels; the numbers are MI355X ray-cast times in frame) ----------------
// cheap steps a lane may take before the wave serves the lanes waiting for a trilinear read.  Round 4 (config 2 / 3 / 5 ray cast):
// 1: 37.7-38.5 us, 2: 37.1-37.7 / c3 +2.6 % frames/s, 3: 38.1-38.3, 4 (rounds 2-3): 38.0-38.8, 6: 40.3
constexpr int kMarchBurst = 2;
// a ray that has just taken this many "block not found" steps in a row is crossing empty space (a silhouette ray on its way from
// the sphere to the wall): phase 1 of the ray-cast workgroup parks it, phase 2 marches the parked rays in waves of their own.
// Config 2 / config 5, one-phase kernel 60.4 / 132.5 us: streak 4: 76 / 152, 6: 62, 8: 54 / 129, 10: 53 / 123, 12: 53 / 117,
// 16: 55 / 118, 24: 58 / 120 -- parking too early also catches rays that only skip a few blocks.
constexpr int kParkStreak = 12;
// directory cells fetched together per round trip by a parked ray's empty-space run (round 2: 4: 55 us, 6: 53, 8: 53; round 4 with a march
// burst of 2, config 2 / config 5 ray cast: 6: 37.2-37.7 / 116-118, 8: 35.8-36.9 / 114.7-114.9, 12: 35.5-36.7 / 112.8-113.1, 16: 40.2-40.6 / 119.6,
// 20: 41.8 / 130, 24: 40.4-42.1 / 131).  Re-swept with the 30-instruction cell (profiles/raycast_lookahead_notes.md, headline frames/s,
// 12: 13 636-13 733): 8: 13 627-13 764, 16: 13 568-13 601 (and 96-100 VGPRs)
constexpr int kParkedLookahead = 12;
// phase 1: "not found" steps in a row after which a ray counts as inside a run for the wave-wide look-ahead, and the cells it fetches
// (re-swept likewise: 8 cells 13 376-13 468, 10: 13 636-13 733, 12: 13 629-13 749; a park streak of 10: 13 683-13 742)
constexpr int kProbeAt = 2;
constexpr int kProbeCells = 10;
// Dense volumes: voxels fetched together by a ray that is crossing free space.  BASELINE configs[2] starts every ray 0.2 m in front
// of the camera and the surface is 1.3-2.3 m away: ~65-115 steps of mu / voxelSize voxels through voxels that read exactly 1 (free
// or never seen), each a dependent round trip.  Measured (config 3 ray cast, event timers): none 90.6 us, 4 voxels 86.6, 8: 92.5,
// 12: 94.0, 16: 103.7 -- the run is NOT what bounds the dense ray cast (its neighbouring rays read the same lines from L2); kept at 4.
// Round 5, with all loads of a look-ahead really in flight together (far_run): 4: 70.7-71.3 us, 6: > 75, 8: 75.3-75.7.
constexpr int kDenseLookahead = 4;

#if ITM_EXP_WAVE_TIMING
static __device__ unsigned long long g_waveStats[8192 * 12];
static __device__ unsigned long long g_waveTrace[160 * 64 * 4];  // waves with index % 32 == 1: per iteration (t0-start, near end, tri end, iteration end | lanes<<48)
#define ITM_WT(...) __VA_ARGS__
__device__ inline unsigned long long wt_wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
  return v;
}
__device__ inline unsigned long long wt_clock() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t = clock64(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); return t; }
#else
#define ITM_WT(...)
#endif

struct RayParams {
  Mat4 invM;
  float ifx, ify, cx, cy;   // (1/fx, 1/fy, cx, cy)
  float oneOverVoxel, mu, voxelSize;
  float lx, ly, lz;         // light source = -(invM column 2)
  int W, H;
};

// Ray set-up shared by both loops: start point, direction and the [total, totalMax) range in voxel units.
struct RaySetup { float px, py, pz, dx, dy, dz, total, totalMax; };

__device__ inline RaySetup ray_setup(int x, int y, const RayParams& p, float2 mm) {
  RaySetup r;
  float pcz = mm.x;
  float pcx = pcz * (((float)x - p.cx) * p.ifx);
  float pcy = pcz * (((float)y - p.cy) * p.ify);
  float acc = 0.0f; acc += pcx * pcx; acc += pcy * pcy; acc += pcz * pcz;
  r.total = sqrtf(acc) * p.oneOverVoxel;
  Vec3 t = transform_point(p.invM, pcx, pcy, pcz);
  const float sx = t.x * p.oneOverVoxel, sy = t.y * p.oneOverVoxel, sz = t.z * p.oneOverVoxel;
  pcz = mm.y;
  pcx = pcz * (((float)x - p.cx) * p.ifx);
  pcy = pcz * (((float)y - p.cy) * p.ify);
  acc = 0.0f; acc += pcx * pcx; acc += pcy * pcy; acc += pcz * pcz;
  r.totalMax = sqrtf(acc) * p.oneOverVoxel;
  t = transform_point(p.invM, pcx, pcy, pcz);
  float dx = t.x * p.oneOverVoxel - sx, dy = t.y * p.oneOverVoxel - sy, dz = t.z * p.oneOverVoxel - sz;
  const float dn = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
  r.dx = dx * dn; r.dy = dy * dn; r.dz = dz * dn;
  r.px = sx; r.py = sy; r.pz = sz;
  return r;
}

// castRay restructured as two nested loops ("while-while"): the inner loop only does the cheap part of a
// step (nearest-voxel read, empty-space / far-field advance) and a lane leaves it as soon as its value lies
// inside the truncation band; the expensive trilinear read (band steps and the post-hit refinement alike)
// sits after the inner loop.  SIMT reconvergence then does the scheduling: lanes that need a trilinear
// read wait while the other lanes of the wave take up to kMarchBurst cheap steps, then the
// trilinear code runs once for all of them -- instead of once per iteration in which ANY lane happens to
// be in the band.  Per ray the sequence of positions, reads and float operations is exactly that of
// the reference's loop (DeviceAgnostic/ITMVisualisationEngine.h:92-158), so results are bit-identical.
//
// Measured on MI355X (config 2, tools/wave_stats.py per-wave cycle traces): the kernel lasts as long as its
// slowest wave (rays that pass the sphere and run ~45 empty-space steps to the wall); a cold voxel/hash
// line costs ~2 000 cycles per dependent round trip, a trilinear step ~4 500.  Burst 1 (= the plain loop)
// 69 us, 2: 65, 3: 64, 4: 62, 8: 66, unbounded: 95 (lanes then serialise each other's empty-space runs).
// The other restructurings that were tried and dropped are listed with their numbers in DESIGN.md section 5.
// One look-ahead round of a far-field run in a DENSE volume.  A ray whose single-voxel read returned exactly 1 steps by
// max(1 * stepScale, 1) voxels and, in free space, reads 1 again: the voxels of the next K positions -- q0 = pt, q1 = pt + step dir,
// ..., each computed with the reference's own operations -- are fetched together and the ray advances over as many of them as
// read exactly 1 (the reference's step for such a value, with its length update and range test); it stops in front of the first
// other value (or position outside the volume), which the regular loop then reads again.  K dependent round trips become one.
// Returns the number of steps taken.
template <class VX, int K>
__device__ inline int far_run(const VolumeView& vol, bool runner, float& px, float& py, float& pz, float& total, float dx, float dy, float dz,
                              float stepScale, float totalMax, bool& ended) {
  const float one = 1.0f * stepScale;                       // sdf * stepScale with sdf == 1
  const float step = (one < 1.0f) ? 1.0f : one;
  const float sx = step * dx, sy = step * dy, sz = step * dz;
  const float farRaw = VX::kShort ? 32767.0f : 1.0f;
  // bit j set: q_j holds something else than exactly 1 (or lies outside the volume, or the lane is no runner): the run stops in front of it.
  // EVERY value goes into the mask, so all K loads are in flight together: with the values consumed one by one in an accept / break
  // chain the compiler sinks the last load into the chain (it is only needed when all others were accepted), i.e. one more dependent
  // round trip in exactly the common case of a run through free space (found in the ISA, round 5).
  uint32_t stop = 0;
  {
    float qx = px, qy = py, qz = pz;
    uint32_t at[K];
    bool in[K];
    float raw[K];
    // (all addresses first, then all loads: interleaved, the register allocator reused a load's destination inside the next address's
    // 64-bit multiply-add and the wave waited for the load there)
#pragma unroll
    for (int j = 0; j < K; ++j) {
      at[j] = dense_lin(vol, (uint32_t)((int)round_ref(qx) - vol.ox), (uint32_t)((int)round_ref(qy) - vol.oy), (uint32_t)((int)round_ref(qz) - vol.oz), in[j], runner);
      qx += sx; qy += sy; qz += sz;
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < K; ++j) raw[j] = VX::load_raw_sdf(vol.vba, (size_t)at[j]);   // voxel 0 / no use for the others
#pragma unroll
    for (int j = 0; j < K; ++j) stop |= (((raw[j] != farRaw) | !in[j]) ? 1u : 0u) << j;      // outside the volume / no runner: stops the run
  }
  const int n = runner ? __builtin_ctz(stop | (1u << K)) : 0;      // positions that read exactly 1, counted from the first
  int taken = 0;
  while (taken < n) {
    px += sx; py += sy; pz += sz; total += step;               // the reference's step for a value of exactly 1, with its length update ...
    ++taken;
    if (!(total < totalMax)) { ended = true; break; }         // ... and its range test
  }
  return taken;
}

// a parked ray: where it stands and how far it has come; direction, end of range etc. are recomputed from the pixel
struct RayResume { float px, py, pz, total; };

// castRay restructured as two nested loops ("while-while"), resumable.
//   LOOKAHEAD > 0 (hash index with the block directory): after a "block not found" step the directory cells of the next K
//     positions of the ray -- computed with the reference's own additions, pt += 8 dir -- are fetched together and the ray
//     advances over as many of them as are empty: K dependent round trips become one.  In a wave where only SOME lanes cross
//     empty space this loses (every lane pays the K classifications and loads: 61 -> 64 / 69 / 77 us for K = 3 / 6 / 10, gated or
//     not); in a wave of nothing but such rays it is what makes their ~45-step runs cheap.
//   PARK: the ray stops (parked = true, returns its position and length in xyz / w) once it has taken kParkStreak
//     "not found" steps in a row; the caller appends it to the queue of the second pass.
// Per ray the sequence of positions, reads and float operations is that of the reference, whatever the pass structure.
// (march_segment, at the end of this file, is the twin of march_ray<VX, DENSE, 0, false> for rays that are not pixels: a change to the
// step, the band or the refinement here has to be made there too.)
template <class VX, bool DENSE, int LOOKAHEAD, bool PARK, class VOL = VolumeView>
__device__ inline float4 march_ray(int x, int y, const VOL& vol, const RayParams& p, float2 mm, const RayResume* resume, bool& parked) {
  // MARCH: next read is a single voxel; TRI: a single-voxel read found the band, the trilinear read of the same position is
  // due; REFINE: the surface was crossed
  enum : int { MARCH = 0, TRI = 1, REFINE = 2, DONE = 4 };
  const float stepScale = p.mu * p.oneOverVoxel;
  const RaySetup r = ray_setup(x, y, p, mm);
  float px = r.px, py = r.py, pz = r.pz, total = r.total;
  const float dx = r.dx, dy = r.dy, dz = r.dz, totalMax = r.totalMax;
  int missStreak = 0;
  if (resume) { px = resume->px; py = resume->py; pz = resume->pz; total = resume->total; missStreak = kParkStreak; }
  BlockCache cache;
  bool found;
  float w = 0.0f;
  parked = false;
  int st = (total < totalMax) ? MARCH : DONE;
  // one forward step of the march loop for a value that is not in the band (or a trilinear value): returns the next state
  auto advance = [&](bool fnd, float sdf) -> int {
    float step;
    int next = MARCH;
    if (!fnd) step = (float)kBlockSide;
    else if (sdf <= 0.0f) { step = sdf * stepScale; next = REFINE; }          // surface crossed: first refinement move, no length update
    else { const float s = sdf * stepScale; step = (s < 1.0f) ? 1.0f : s; }
    px += step * dx; py += step * dy; pz += step * dz;
    if (next != REFINE) { total += step; if (!(total < totalMax)) next = DONE; }
    return next;
  };
  // One look-ahead round of an empty-space run (hash index with the block directory): the directory cells of the positions q0 = pt,
  // q1 = pt + 8 dir, ... -- computed with the reference's own additions -- are fetched together (every lane loads, a lane that is no
  // runner ignores what it gets) and the ray advances over as many of them as are empty, each the reference's step for a position without a block, with
  // its length update and range test; it stops in front of the first position that holds a block (or lies outside the directory),
  // which the regular loop then reads.  Returns the number of steps taken.
  auto miss_run = [&](auto kc, bool runner) -> int {
    constexpr int K = decltype(kc)::value;
    const float sx = (float)kBlockSide * dx, sy = (float)kBlockSide * dy, sz = (float)kBlockSide * dz;   // exact products
    // (Round 5: with every cell folded into one mask -- all K loads awaited together, the count taken with a find-first-bit -- the hash
    // ray cast got SLOWER, configs[1] 36.5 -> 37.3 us, configs[4] 111.5 -> 119 us: the chain below consumes the cells as they arrive and
    // leaves at the first block.  profiles/r5_raycast_notes.md)
    // A cell is 30 straight-line instructions (40 and an exec bracket before: ray cast 36.4 -> 34.8 us, config 5's 112 -> 107.5 us,
    // profiles/raycast_lookahead_notes.md; a parked wave has its SIMD to itself and pays every instruction and every exec bracket of
    // a cell with issue time):
    //  * the index comes from the voxel-unit coordinate t = voxel - 8 * origin (dir_cell_voxel: six bit-field extracts, no shift to
    //    block units) and is a valid cell for EVERY t, so the load is unconditional -- no select of the index, which the compiler
    //    turned into an exec-masked bracket around the index arithmetic of every cell;
    //  * whether the directory covers the round is asked ONCE: a ray's positions are monotone per axis (additions of one sign, a monotone
    //    rounding), so a round whose first and last cell lie inside the cube lies inside it entirely.  A round that touches the cube's
    //    face takes no step at all; the regular loop reads those positions through the table, as it does everywhere outside the cube;
    //  * the loads are pinned in front of the chain: without its bracket a load is free to sink into the chain, behind the test of the
    //    cell before it, and the K round trips are dependent again (measured: 13 400 -> 12 900 frames/s).  The empty asm with its memory
    //    clobber keeps every load above it; the scheduling fence per cell keeps the addresses from being computed all at once (110-120
    //    VGPRs, four waves per SIMD); the asm on `edge` has the first cell's coordinates folded before the loop goes on.
    static_assert(K >= 1 && K <= 32, "look-ahead cells");
    int ahead[K];
    uint32_t edge = 0;      // the first and the last cell's cube-relative voxel coordinates, or-ed
    {
      float qx = px, qy = py, qz = pz;
      const uint32_t ox8 = (uint32_t)vol.org.dx * (uint32_t)kBlockSide, oy8 = (uint32_t)vol.org.dy * (uint32_t)kBlockSide, oz8 = (uint32_t)vol.org.dz * (uint32_t)kBlockSide;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const uint32_t tx = (uint32_t)(int)round_ref(qx) - ox8, ty = (uint32_t)(int)round_ref(qy) - oy8, tz = (uint32_t)(int)round_ref(qz) - oz8;
        const uint32_t at = dir_cell_voxel(tx, ty, tz) << 2;                       // (a 32-bit byte offset from the scalar base)
        if (j == 0 || j == K - 1) { edge |= tx | ty | tz; asm volatile("" : "+v"(edge)); }
        ahead[j] = *(const int32_t*)((const char*)vol.dirPtr + at);
        __builtin_amdgcn_sched_barrier(0);
        qx += sx; qy += sy; qz += sz;
      }
    }
    asm volatile("" ::: "memory");
    int taken = 0;
    if (runner && dir_covers_voxel(edge, 0u, 0u)) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (ahead[j] >= 0) break;                             // q_j holds a block: regular read next
        px += sx; py += sy; pz += sz; total += (float)kBlockSide;   // the reference's step for a position without a block
        ++taken;
        if (!(total < totalMax)) { st = DONE; break; }
      }
    }
    return taken;
  };
  ITM_WT(const unsigned long long wtStart = wt_clock(); unsigned wtOuter = 0;)
  bool missed = false;      // DENSE: the last single-voxel read found no voxel
  while (st != DONE) {
    if constexpr (DENSE) {
      // A ray that has LEFT the volume -- outside on an axis along which it moves away -- never comes back (its coordinate on that
      // axis only grows in magnitude, additions of one sign are monotone in float arithmetic too, and so is the rounding of the
      // look-up): every further read finds nothing and the reference takes its 8-voxel step until the range ends.  Once every lane
      // of the wave is done or gone, those steps are taken here without the look-ups: the same additions in the same order, ~6
      // instructions instead of ~35 per step (BASELINE configs[2]: the wall lies behind the volume, its rays take ~30 such steps).
      if (__any(missed)) {
        bool gone = false;
        if (st == MARCH && missed) {
          const int ix = (int)round_ref(px) - vol.ox, iy = (int)round_ref(py) - vol.oy, iz = (int)round_ref(pz) - vol.oz;
          gone = (ix >= vol.sx && dx >= 0.0f) || (ix < 0 && dx <= 0.0f) || (iy >= vol.sy && dy >= 0.0f) || (iy < 0 && dy <= 0.0f) ||
                 (iz >= vol.sz && dz >= 0.0f) || (iz < 0 && dz <= 0.0f);
        }
        if (__all(st == DONE || gone)) {
          const float step = (float)kBlockSide;
          const float sx = step * dx, sy = step * dy, sz = step * dz;        // the products of advance(false, .)
          while (st == MARCH) {
            px += sx; py += sy; pz += sz;
            total += step;
            if (!(total < totalMax)) st = DONE;
          }
          break;
        }
      }
    }
    ITM_WT(const unsigned long long wt0 = wt_clock(); unsigned wtInner = 0; const unsigned wtLanes0 = __popcll(__ballot(1)); const unsigned wtMarch0 = __popcll(__ballot(st == MARCH));)
    // ---- cheap phase: at most kMarchBurst single-voxel steps, so that waiting lanes are served regularly ----
    int budget = kMarchBurst;
    while (st == MARCH && budget > 0) {
      --budget;
      ITM_WT(++wtInner;)
      const float sdf = sdf_nearest<VX, DENSE>(vol, px, py, pz, found, cache);
      {
        // the step as selects rather than branches (the same operations on the same values as advance(); a lone wave pays every
        // taken or skipped branch of a step with issue bubbles, profiles/r3_raycast_notes.md)
        const bool band = found && (sdf <= 0.1f) && (sdf >= -0.5f);       // the position is kept for the trilinear read
        const bool crossed = found && (sdf <= 0.0f);                      // (below the band) first refinement move, no length update
        const float s = sdf * stepScale;
        const float fwd = (s < 1.0f) ? 1.0f : s;
        const float step = found ? (crossed ? s : fwd) : (float)kBlockSide;
        const float nx = px + step * dx, ny = py + step * dy, nz = pz + step * dz, nt = total + step;
        px = band ? px : nx; py = band ? py : ny; pz = band ? pz : nz;
        total = (band || crossed) ? total : nt;
        st = band ? TRI : crossed ? REFINE : (total < totalMax) ? MARCH : DONE;
      }
      if constexpr (DENSE) missed = !found;
      if constexpr (DENSE && LOOKAHEAD > 0) {
        // (Several look-aheads back to back while all of their positions read exactly 1 -- no single-voxel read in between -- were
        // measured in round 5: config 3's ray cast 71 us with one, 79 with two, 95 with four, 120 with eight: the lanes of the wave that
        // are near the surface wait through the others' runs.  profiles/r5_raycast_notes.md)
        const bool far = st == MARCH && found && sdf == 1.0f;      // SDF_valueToFloat(32767) is exactly 1
        if (__any(far)) {
          bool ended = false;
          (void)far_run<VX, LOOKAHEAD>(vol, far, px, py, pz, total, dx, dy, dz, stepScale, totalMax, ended);
          if (ended) st = DONE;
        }
      }
      if constexpr (!DENSE && (PARK || LOOKAHEAD > 0)) missStreak = found ? 0 : missStreak + 1;
      if constexpr (!DENSE && PARK && kProbeCells > 0) {
        // phase 1, once the wave has nothing left to march but rays inside "not found" runs (the other lanes are done or wait for their
        // trilinear read): those rays look kProbeCells positions ahead together, one round trip for the whole wave
        const bool runner = st == MARCH && missStreak >= kProbeAt;
        if (vol.dirPtr && __all(st != MARCH || runner) && __any(runner)) {
          const int adv = miss_run(std::integral_constant<int, kProbeCells>(), runner);
          if (runner) missStreak += adv;
        }
      }
      if constexpr (!DENSE && PARK) {
        if (st == MARCH && missStreak >= kParkStreak) { parked = true; st = DONE; }
      }
      if constexpr (!DENSE && LOOKAHEAD > 0) {
        if (vol.dirPtr && __any(missStreak >= kParkStreak && st == MARCH))
          (void)miss_run(std::integral_constant<int, (LOOKAHEAD > 0 ? LOOKAHEAD : 1)>(), missStreak >= kParkStreak && st == MARCH);
      }
    }
    ITM_WT(const unsigned long long wtA = wt_clock(); const unsigned wtTriLanes = __popcll(__ballot(st == TRI || st == REFINE)); wtInner = (unsigned)wt_wave_max(wtInner);)
    // ---- expensive phase: one 2x2x2 fetch for every lane that waits for one ---------------------------------------------
    if (st == TRI || st == REFINE) {
      Corners<VX, DENSE> cn;
      cn.fetch(vol, px, py, pz, cache);
      if (st == REFINE) {
        const float step = cn.trilinear() * stepScale;
        px += step * dx; py += step * dy; pz += step * dz;
        w = 1.0f; st = DONE;
      } else {
        st = advance(true, cn.trilinear());
      }
    }
    ITM_WT({ const float keep2 = total + px; asm volatile("" :: "v"(keep2)); const unsigned long long tB = wt_clock();
      const unsigned wv = blockIdx.x * 4 + (threadIdx.x >> 6);
#ifdef ITM_EXP_TRACE_TILE0
      // trace the four waves of 40 consecutive tiles starting at ITM_EXP_TRACE_TILE0, first pass only
      const bool wtPick = !resume && wv >= 4u * ITM_EXP_TRACE_TILE0 && wv < 4u * ITM_EXP_TRACE_TILE0 + 160u;
      const unsigned wtSlot = wv - 4u * ITM_EXP_TRACE_TILE0;
#else
      const bool wtPick = (wv & 31) == 1 && (wv >> 5) < 160;
      const unsigned wtSlot = wv >> 5;
#endif
      if (wtPick && wtOuter < 64) { unsigned long long* tr = g_waveTrace + ((size_t)wtSlot * 64 + wtOuter) * 4; tr[0] = wt0 - wtStart; tr[1] = wtA - wtStart; tr[2] = tB - wtStart; tr[3] = wtLanes0 | (wtMarch0 << 8) | (wtTriLanes << 16) | (wtInner << 24); }
      ++wtOuter; })
  }
#if ITM_EXP_WAVE_TIMING
  {
    const unsigned long long wtEnd = wt_clock();
    const unsigned wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned long long mOuter = wt_wave_max(wtOuter);
    if ((threadIdx.x & 63) == 0 && wv < 8192) { unsigned long long* o = g_waveStats + (size_t)wv * 12; o[0] = wtEnd - wtStart; o[1] = mOuter; }
  }
#endif
  if (PARK && parked) return make_float4(px, py, pz, total);
  return make_float4(px, py, pz, w);
}

// castRay for callers that want one ray start to finish
template <class VX, bool DENSE, class VOL = VolumeView>
__device__ inline float4 cast_ray(int x, int y, const VOL& vol, const RayParams& p, float2 mm) {
  bool parked;
  return march_ray<VX, DENSE, 0, false>(x, y, vol, p, mm, nullptr, parked);
}

// castRay from a GIVEN set-up, for rays that are not pixels of a frame (query.hip): what march_ray<VX, DENSE, 0, false> does after its
// ray_setup -- the same two nested loops, the same reads and float operations per ray -- without anything collective over the wave
// (look-ahead, parking, the dense "every lane has left the volume" exit): neighbouring lanes are unrelated rays.  A function of its own
// rather than a split of march_ray: with the split the frame ray-cast kernels kept their registers, scratch and occupancy but came out
// with their instructions in another order (a few s_waitcnt / s_nop more or fewer), and those kernels are tuned to the microsecond.
template <class VX, bool DENSE, class VOL = VolumeView>
__device__ inline float4 march_segment(const RaySetup& r, float stepScale, const VOL& vol) {
  enum : int { MARCH = 0, TRI = 1, REFINE = 2, DONE = 4 };
  float px = r.px, py = r.py, pz = r.pz, total = r.total;
  const float dx = r.dx, dy = r.dy, dz = r.dz, totalMax = r.totalMax;
  BlockCache cache;
  bool found;
  float w = 0.0f;
  int st = (total < totalMax) ? MARCH : DONE;
  while (st != DONE) {
    // ---- cheap phase: at most kMarchBurst single-voxel steps (march_ray's step, as selects) ----
    int budget = kMarchBurst;
    while (st == MARCH && budget > 0) {
      --budget;
      const float sdf = sdf_nearest<VX, DENSE>(vol, px, py, pz, found, cache);
      const bool band = found && (sdf <= 0.1f) && (sdf >= -0.5f);       // the position is kept for the trilinear read
      const bool crossed = found && (sdf <= 0.0f);                      // (below the band) first refinement move, no length update
      const float s = sdf * stepScale;
      const float fwd = (s < 1.0f) ? 1.0f : s;
      const float step = found ? (crossed ? s : fwd) : (float)kBlockSide;
      const float nx = px + step * dx, ny = py + step * dy, nz = pz + step * dz, nt = total + step;
      px = band ? px : nx; py = band ? py : ny; pz = band ? pz : nz;
      total = (band || crossed) ? total : nt;
      st = band ? TRI : crossed ? REFINE : (total < totalMax) ? MARCH : DONE;
    }
    // ---- expensive phase: one 2x2x2 fetch for every lane that waits for one ----
    if (st == TRI || st == REFINE) {
      Corners<VX, DENSE> cn;
      cn.fetch(vol, px, py, pz, cache);
      const float sdf = cn.trilinear();
      if (st == REFINE) {
        const float step = sdf * stepScale;
        px += step * dx; py += step * dy; pz += step * dz;
        w = 1.0f; st = DONE;
      } else if (sdf <= 0.0f) {                                         // surface crossed: first refinement move, no length update
        const float step = sdf * stepScale;
        px += step * dx; py += step * dy; pz += step * dz;
        st = REFINE;
      } else {
        const float s = sdf * stepScale;
        const float step = (s < 1.0f) ? 1.0f : s;
        px += step * dx; py += step * dy; pz += step * dz;
        total += step;
        st = (total < totalMax) ? MARCH : DONE;
      }
    }
  }
  return make_float4(px, py, pz, w);
}

}  // namespace itm
