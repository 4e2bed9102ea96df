// mesh_smooth.hip -- lambda|mu (Taubin) and Laplacian smoothing of the indexed mesh (mesh_index.hip), in fixed point.
//
// The reference's ITMMesh is a triangle buffer and nothing else; a TSDF mesh carries stair-steps and per-voxel noise on every surface,
// and every host smooths it before it shows or saves it.  Defined on the present index (include/itm_hip.h): a proper triangle gives
// each corner one neighbour entry per other corner, positions are quantised once to int32, every pass is the rounded mean offset of
// the entries times a Q16 factor in int64, all vertices at once from the previous iterate, and the result is dequantised once.
// Integers only: the result does not depend on the order in which lanes ran, on the order inside a row or on the kernel form.
//
// MI355X design.
//   1. Adjacency, once per call, as CSR: smooth_count_kernel adds 2 per corner of every proper triangle with integer atomics; the
//      exclusive prefix is taken per chunk of 1024 vertices (chunk sums, a carry scan of the sums by one workgroup -- ordered_device.h
//      --, then a workgroup scan per chunk); smooth_fill_kernel writes a corner's two entries at an atomic cursor of its row.  Rows
//      have room for 6 entries per triangle, so nothing travels to the host in between.
//   2. Topology: one lane per vertex counts every entry's multiplicity in its row (O(n^2); the median n is 12): a row of up to
//      kRegisterRow entries is read once and compared in registers, a longer one is walked in memory.  Rows above
//      kHeavyRow entries (a fan apex) are listed and go to one wave per row, the lanes striding over the entries, a launch later.
//      The three counts and the maximum are aggregated per workgroup, of which the launch has at most kTopologyBlocks, before they
//      reach the counters: one word takes some 90 atomics a microsecond, and a set per wave (19 000 on the largest test mesh) cost
//      that call more than 100 microseconds (profiles/mesh_smooth_notes.md).
//   3. Quantise into the first of two ping-pong arrays of int4: 16 bytes per vertex, one dwordx4 gather per neighbour.  Input that
//      is out of range or not finite raises counters[4]; the launches that write into the mesh read that word -- a kernel boundary
//      later -- and leave at once, and the host reads it with the statistics: one wait per call.
//   4. One launch per pass.  The kernel boundary is what makes the previous iterate visible across the eight XCDs' L2s: nothing here
//      rests on a load inside a launch being fresh (mesh_components.hip's header has the argument), and passes are not fused.
//      Gather form: one lane per vertex, int64 sums in registers.  Vertices are numbered by first occurrence in a block-ordered
//      buffer, so a row's neighbours are close in index and the gathers hit the L2.  The waves of the same launch then take the
//      heavy rows, one wave per row.
//      Scatter form (ITM_DEBUG_MESH_SMOOTH_SCATTER): one lane per proper triangle adds, per corner, the sum of the other two corners
//      into that vertex's int64 accumulators with 64-bit integer atomics; a second launch applies the step and clears them.  The
//      same bits by construction; the cross-check and the measured alternative (profiles/mesh_smooth_notes.md).
//   5. smooth_finish_kernel dequantises the moving vertices in place and rewrites the soup through the faces in the same launch: a
//      soup vertex of a moving vertex is computed from the last iterate, of any other copied from the vertex array, which no lane
//      of the launch writes for those.
#include <algorithm>
#include <cmath>

#include "itm_internal.h"
#include "mesh_types.h"
#include "ordered_device.h"
#include "wave_utils.h"

namespace itm {


constexpr uint32_t kHeavyRow = 128;               // rows with more entries go to one wave per row
constexpr int kRegisterRow = 16;                  // rows up to this many entries are judged in registers (the median is 12)
constexpr size_t kTopologyBlocks = 512;           // workgroups of the topology launch, each with one set of atomics at its end
constexpr int kSmoothChunk = 1024;                // vertices per workgroup of the prefix passes
constexpr int kSmoothLimit = 1 << 30;             // |x| <= 2^30 fixed-point units
constexpr uint32_t kIrregular = 1u, kIsolated = 2u, kMoving = 4u;
enum { kCountMoving = 0, kCountIrregular, kCountIsolated, kCountMaxEntries, kCountBad, kCountHeavy, kSmoothCounters = 8 };
static_assert(sizeof(itm_mesh_smooth_config) == 32 && sizeof(itm_mesh_smooth_stats) == 32, "the smoothing records are 32 bytes each");

__device__ inline bool proper(uint32_t a, uint32_t b, uint32_t c) { return a != b && a != c && b != c; }

// floor(num / den), den > 0.  The operands of a mesh fit 32 bits nearly always: the 64-bit division is the exception.
__device__ inline long long floor_div(long long num, long long den) {
  if (num >= -0x7fffffffll && num <= 0x7fffffffll && den <= 0x7fffffffll) {
    const int n = (int)num, d = (int)den;
    const int q = n / d;
    return (long long)(q - ((n % d != 0 && n < 0) ? 1 : 0));
  }
  const long long q = num / den;
  return q - ((num % den != 0 && num < 0) ? 1 : 0);
}

// One coordinate of one pass: S the sum over the n > 0 entries, f the factor in Q16.  n <= 2 noTriangles < 2^31 * 2 / 3 and
// |x| <= 2^30, so |a| <= n * 2^31 and 2 |a| + n < 2^63; |d| <= 2^31 + 1 and |f| <= 2^16.
__device__ inline int smooth_step(int x, long long S, long long n, long long f) {
  const long long a = S - n * (long long)x;
  const long long d = floor_div(2 * a + n, 2 * n);
  const long long s = (f * d + 32768) >> 16;
  long long r = (long long)x + s;
  r = r < -(long long)kSmoothLimit ? -(long long)kSmoothLimit : r;
  r = r > (long long)kSmoothLimit ? (long long)kSmoothLimit : r;
  return (int)r;
}

__device__ inline int4 smooth_step3(int4 p, long long sx, long long sy, long long sz, uint32_t n, int f) {
  return make_int4(smooth_step(p.x, sx, n, f), smooth_step(p.y, sy, n, f), smooth_step(p.z, sz, n, f), 0);
}

__device__ inline long long wave_sum64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---- adjacency ------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) smooth_count_kernel(const uint32_t* __restrict__ faces, uint32_t nT, uint32_t* __restrict__ rowCount) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nT; i += gridDim.x * 256u) {
    const uint32_t a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    if (!proper(a, b, c)) continue;
    atomicAdd(rowCount + a, 2u); atomicAdd(rowCount + b, 2u); atomicAdd(rowCount + c, 2u);
  }
}

__global__ void __launch_bounds__(256) smooth_chunk_sum_kernel(const uint32_t* __restrict__ rowCount, uint32_t nV, uint32_t* __restrict__ chunkSum) {
  __shared__ int lds[4];
  int n = 0;
#pragma unroll
  for (int i = 0; i < kSmoothChunk / 256; ++i) {
    const uint32_t k = blockIdx.x * (uint32_t)kSmoothChunk + i * 256u + threadIdx.x;
    n += k < nV ? (int)rowCount[k] : 0;
  }
  const int sum = block_reduce_sum<4>(n, lds);
  if (threadIdx.x == 0) chunkSum[blockIdx.x] = (uint32_t)sum;
}

// exclusive scan of the chunk sums (in place) by one workgroup; rowStart[nV] = the number of entries
__global__ void __launch_bounds__(1024) smooth_scan_kernel(uint32_t* __restrict__ chunkSum, int nChunks, uint32_t* __restrict__ rowStart, uint32_t nV) {
  const uint32_t total = carry_scan<16, uint32_t>(nChunks, [&](int i) { return chunkSum[i]; }, [&](int i, uint32_t before) { chunkSum[i] = before; });
  if (threadIdx.x == 0) rowStart[nV] = total;
}

// rowStart[k] = entries of the vertices before k; rowCount[k] = 0: the fill's cursor
__global__ void __launch_bounds__(256) smooth_row_start_kernel(uint32_t* __restrict__ rowCount, uint32_t nV, const uint32_t* __restrict__ chunkSum,
                                                               uint32_t* __restrict__ rowStart) {
  __shared__ int lds[5];
  uint32_t base = chunkSum[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kSmoothChunk / 256; ++i) {
    const uint32_t k = blockIdx.x * (uint32_t)kSmoothChunk + i * 256u + threadIdx.x;
    const int n = k < nV ? (int)rowCount[k] : 0;
    int total;
    const int ex = block_exclusive_scan<4>(n, lds, &total);
    if (k < nV) { rowStart[k] = base + (uint32_t)ex; rowCount[k] = 0u; }
    base += (uint32_t)total;
  }
}

// the order inside a row is that of the cursor's answers: arbitrary, and no result depends on it
__global__ void __launch_bounds__(256) smooth_fill_kernel(const uint32_t* __restrict__ faces, uint32_t nT, const uint32_t* __restrict__ rowStart,
                                                          uint32_t* __restrict__ cursor, uint32_t* __restrict__ entries) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nT; i += gridDim.x * 256u) {
    const uint32_t a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    if (!proper(a, b, c)) continue;
    uint32_t* ra = entries + rowStart[a] + atomicAdd(cursor + a, 2u);
    ra[0] = b; ra[1] = c;
    uint32_t* rb = entries + rowStart[b] + atomicAdd(cursor + b, 2u);
    rb[0] = a; rb[1] = c;
    uint32_t* rc = entries + rowStart[c] + atomicAdd(cursor + c, 2u);
    rc[0] = a; rc[1] = b;
  }
}

// ---- topology -------------------------------------------------------------------------------------------------------------------------

// Called by all 256 threads of a workgroup, once: the workgroup's counts and maximum to the counters.  One word takes some 90 atomics
// a microsecond however many CUs send them, so the counts are summed over the workgroup first and the topology launch is kept to
// kTopologyBlocks workgroups: a few thousand atomics a call, not one set per wave.
__device__ inline void add_topology_counts(uint32_t* counters, uint32_t moving, uint32_t irregular, uint32_t isolated, uint32_t maxEntries) {
  __shared__ uint32_t part[4][4];
  const int m = wave_reduce_sum((int)moving), r = wave_reduce_sum((int)irregular), s = wave_reduce_sum((int)isolated);
  const uint32_t x = wave_reduce_umax(maxEntries);
  if (lane_id() == 0) { uint32_t* p = part[wave_id()]; p[0] = (uint32_t)m; p[1] = (uint32_t)r; p[2] = (uint32_t)s; p[3] = x; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t bm = part[0][0] + part[1][0] + part[2][0] + part[3][0], br = part[0][1] + part[1][1] + part[2][1] + part[3][1];
  const uint32_t bs = part[0][2] + part[1][2] + part[2][2] + part[3][2];
  const uint32_t bx = max(max(part[0][3], part[1][3]), max(part[2][3], part[3][3]));
  if (bm) atomicAdd(counters + kCountMoving, bm);
  if (br) atomicAdd(counters + kCountIrregular, br);
  if (bs) atomicAdd(counters + kCountIsolated, bs);
  if (bx) atomicMax(counters + kCountMaxEntries, bx);
}

__device__ inline uint32_t topology_flags(bool irregular, bool isolated, int pin) {
  return (irregular ? kIrregular : 0u) | (isolated ? kIsolated : 0u) | ((!isolated && !(pin && irregular)) ? kMoving : 0u);
}

// one lane per vertex; a row above kHeavyRow entries is listed in heavy[0 .. counters[kCountHeavy]) and left to the launch after
__global__ void __launch_bounds__(256) smooth_topology_kernel(const uint32_t* __restrict__ rowStart, const uint32_t* __restrict__ entries, uint32_t nV, int pin,
                                                              uint8_t* __restrict__ vertexFlags, uint32_t* __restrict__ heavy, uint32_t capHeavy,
                                                              uint32_t* __restrict__ counters) {
  uint32_t moving = 0u, irregularCount = 0u, isolatedCount = 0u, maxEntries = 0u;
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const uint32_t r0 = rowStart[k], n = rowStart[k + 1] - r0;
    maxEntries = n > maxEntries ? n : maxEntries;
    if (n > kHeavyRow) {
      const uint32_t h = atomicAdd(counters + kCountHeavy, 1u);
      if (h < capHeavy) heavy[h] = k;                                  // (h < capHeavy always: capHeavy * kHeavyRow exceeds the entries)
      continue;
    }
    const uint32_t* row = entries + r0;
    bool irregular = false;
    if (n <= (uint32_t)kRegisterRow) {
      // nearly every row of a marching-cubes mesh: the row is read once into registers and compared there, fully unrolled, so the
      // n^2 comparisons cost no loads and no branches.  Slots past the row hold a value no vertex has (nV < 2^31) and are not judged.
      uint32_t r[kRegisterRow];
#pragma unroll
      for (int j = 0; j < kRegisterRow; ++j) r[j] = (uint32_t)j < n ? row[j] : 0xffffffffu;
#pragma unroll
      for (int i = 0; i < kRegisterRow; ++i) {
        uint32_t times = 0u;
#pragma unroll
        for (int j = 0; j < kRegisterRow; ++j) times += r[j] == r[i] ? 1u : 0u;
        irregular = irregular || ((uint32_t)i < n && times != 2u);
      }
    } else {
      for (uint32_t i = 0; i < n && !irregular; ++i) {
        const uint32_t e = row[i];
        uint32_t times = 0u;
        for (uint32_t j = 0; j < n; ++j) times += row[j] == e ? 1u : 0u;
        irregular = times != 2u;
      }
    }
    const uint32_t f = topology_flags(irregular, n == 0u, pin);
    vertexFlags[k] = (uint8_t)f;
    moving += (f & kMoving) ? 1u : 0u; irregularCount += irregular ? 1u : 0u; isolatedCount += n == 0u ? 1u : 0u;
  }
  add_topology_counts(counters, moving, irregularCount, isolatedCount, maxEntries);   // (every thread arrives: the loop has no barrier)
}

// one wave per listed row: lane l counts the multiplicity of entries l, l + 64, ...; the inner load is the same address in every lane
__global__ void __launch_bounds__(256) smooth_topology_heavy_kernel(const uint32_t* __restrict__ rowStart, const uint32_t* __restrict__ entries, int pin,
                                                                    uint8_t* __restrict__ vertexFlags, const uint32_t* __restrict__ heavy, uint32_t capHeavy,
                                                                    uint32_t* __restrict__ counters) {
  const uint32_t nHeavy = counters[kCountHeavy] < capHeavy ? counters[kCountHeavy] : capHeavy;
  const uint32_t wave = blockIdx.x * 4u + wave_id(), nWaves = gridDim.x * 4u;
  uint32_t moving = 0u, irregularCount = 0u;
  for (uint32_t h = wave; h < nHeavy; h += nWaves) {                     // (uniform over the wave)
    const uint32_t k = heavy[h];
    const uint32_t r0 = rowStart[k], n = rowStart[k + 1] - r0;
    const uint32_t* row = entries + r0;
    bool bad = false;
    for (uint32_t i = lane_id(); i < n && !bad; i += kWave) {
      const uint32_t e = row[i];
      uint32_t times = 0u;
      for (uint32_t j = 0; j < n; ++j) times += row[j] == e ? 1u : 0u;
      bad = times != 2u;
    }
    const bool irregular = __ballot(bad) != 0ull;
    const uint32_t f = topology_flags(irregular, false, pin);
    if (lane_id() == 0) {
      vertexFlags[k] = (uint8_t)f;
      moving += (f & kMoving) ? 1u : 0u; irregularCount += irregular ? 1u : 0u;
    }
  }
  add_topology_counts(counters, moving, irregularCount, 0u, 0u);
}

// ---- the passes -----------------------------------------------------------------------------------------------------------------------

// x[k] = rint(v[k] / quantum) in double, ties to even; counters[kCountBad] where that is not finite or beyond 2^30
__global__ void __launch_bounds__(256) smooth_quantise_kernel(const float* __restrict__ vertices, uint32_t nV, float quantum, int4* __restrict__ x,
                                                              uint32_t* __restrict__ counters) {
  const double q = (double)quantum;
  bool bad = false;
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double r = rint((double)vertices[3 * (size_t)k + a] / q);
      const bool ok = r >= -(double)kSmoothLimit && r <= (double)kSmoothLimit;      // false for a NaN
      bad = bad || !ok;
      c[a] = ok ? (int)r : 0;
    }
    x[k] = make_int4(c[0], c[1], c[2], 0);
  }
  if (bad) atomicOr(counters + kCountBad, 1u);
}

// Gather form of one pass: xn = the step of x.  A row above kHeavyRow entries is summed by one wave in the second half.
__global__ void __launch_bounds__(256) smooth_gather_kernel(const int4* __restrict__ x, int4* __restrict__ xn, const uint32_t* __restrict__ rowStart,
                                                            const uint32_t* __restrict__ entries, const uint8_t* __restrict__ vertexFlags, uint32_t nV, int f,
                                                            const uint32_t* __restrict__ heavy, uint32_t capHeavy, const uint32_t* __restrict__ counters) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const int4 p = x[k];
    if (!(vertexFlags[k] & kMoving)) { xn[k] = p; continue; }
    const uint32_t r0 = rowStart[k], n = rowStart[k + 1] - r0;
    if (n > kHeavyRow) continue;
    long long sx = 0, sy = 0, sz = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const int4 q = x[entries[r0 + i]];
      sx += q.x; sy += q.y; sz += q.z;
    }
    xn[k] = smooth_step3(p, sx, sy, sz, n, f);
  }
  const uint32_t nHeavy = counters[kCountHeavy] < capHeavy ? counters[kCountHeavy] : capHeavy;      // written launches ago
  const uint32_t wave = blockIdx.x * 4u + wave_id(), nWaves = gridDim.x * 4u;
  for (uint32_t h = wave; h < nHeavy; h += nWaves) {                     // (uniform over the wave)
    const uint32_t k = heavy[h];
    if (!(vertexFlags[k] & kMoving)) continue;                           // (copied above)
    const uint32_t r0 = rowStart[k], n = rowStart[k + 1] - r0;
    long long sx = 0, sy = 0, sz = 0;
    for (uint32_t i = lane_id(); i < n; i += kWave) {
      const int4 q = x[entries[r0 + i]];
      sx += q.x; sy += q.y; sz += q.z;
    }
    sx = wave_sum64(sx); sy = wave_sum64(sy); sz = wave_sum64(sz);
    if (lane_id() == 0) xn[k] = smooth_step3(x[k], sx, sy, sz, n, f);
  }
}

// Scatter form, first half: sums[4 k + c] += the other two corners' coordinate c, for every corner k of every proper triangle
__global__ void __launch_bounds__(256) smooth_scatter_kernel(const int4* __restrict__ x, const uint32_t* __restrict__ faces, uint32_t nT,
                                                             unsigned long long* __restrict__ sums) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nT; i += gridDim.x * 256u) {
    const uint32_t a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    if (!proper(a, b, c)) continue;
    const int4 pa = x[a], pb = x[b], pc = x[c];
    const uint32_t v[3] = {a, b, c};
    const long long s[3][3] = {{(long long)pb.x + pc.x, (long long)pb.y + pc.y, (long long)pb.z + pc.z},
                               {(long long)pa.x + pc.x, (long long)pa.y + pc.y, (long long)pa.z + pc.z},
                               {(long long)pa.x + pb.x, (long long)pa.y + pb.y, (long long)pa.z + pb.z}};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int axis = 0; axis < 3; ++axis) atomicAdd(sums + 4 * (size_t)v[k] + axis, (unsigned long long)s[k][axis]);   // (two's complement: the signed sum)
  }
}

// Scatter form, second half: the step from the accumulated sums, which are cleared for the next pass
__global__ void __launch_bounds__(256) smooth_apply_kernel(const int4* __restrict__ x, int4* __restrict__ xn, const uint32_t* __restrict__ rowStart,
                                                           const uint8_t* __restrict__ vertexFlags, uint32_t nV, int f, long long* __restrict__ sums) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const int4 p = x[k];
    const uint32_t n = rowStart[k + 1] - rowStart[k];
    long long* s = sums + 4 * (size_t)k;
    if ((vertexFlags[k] & kMoving) && n) xn[k] = smooth_step3(p, s[0], s[1], s[2], n, f);
    else xn[k] = p;
    s[0] = 0; s[1] = 0; s[2] = 0;
  }
}

__device__ inline float dequantise(int x, double q) { return (float)((double)x * q); }

// The moving vertices dequantised in place, and the soup through the faces (soup == nullptr: the hook has none).  Nothing is written
// when the input was refused.
__global__ void __launch_bounds__(256) smooth_finish_kernel(const int4* __restrict__ x, const uint8_t* __restrict__ vertexFlags, uint32_t nV, float quantum,
                                                            float* vertices, const uint32_t* __restrict__ faces, uint32_t nSoup, float* __restrict__ soup,
                                                            const uint32_t* __restrict__ counters) {
  if (counters[kCountBad] != 0u) return;
  const double q = (double)quantum;
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    if (!(vertexFlags[k] & kMoving)) continue;
    const int4 p = x[k];
    vertices[3 * (size_t)k] = dequantise(p.x, q); vertices[3 * (size_t)k + 1] = dequantise(p.y, q); vertices[3 * (size_t)k + 2] = dequantise(p.z, q);
  }
  if (!soup) return;
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < nSoup; j += gridDim.x * 256u) {
    const uint32_t k = faces[j];
    float* o = soup + 3 * (size_t)j;
    if (vertexFlags[k] & kMoving) {                                      // from the iterate: this launch is still writing vertices[k]
      const int4 p = x[k];
      o[0] = dequantise(p.x, q); o[1] = dequantise(p.y, q); o[2] = dequantise(p.z, q);
    } else {                                                             // no lane writes vertices[k]: its own 96 bits
      const uint32_t* s = (const uint32_t*)vertices + 3 * (size_t)k;
      uint32_t* ow = (uint32_t*)o;
      ow[0] = s[0]; ow[1] = s[1]; ow[2] = s[2];
    }
  }
}

static int grid_for(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 2048); }

static int check_smooth_config(const itm_mesh_smooth_config* cfg) {
  if (!cfg) return set_error(ITM_ERR_INVALID, "null argument");
  if (cfg->steps > (uint32_t)ITM_MESH_SMOOTH_MAX_STEPS) return set_error(ITM_ERR_INVALID, "mesh smoothing: more than ITM_MESH_SMOOTH_MAX_STEPS passes");
  if (cfg->lambdaQ16 > 65536 || cfg->lambdaQ16 < -65536 || cfg->muQ16 > 65536 || cfg->muQ16 < -65536)
    return set_error(ITM_ERR_INVALID, "mesh smoothing: |lambdaQ16| and |muQ16| are at most 65536");
  if (!(cfg->quantum > 0.0f) || !std::isfinite(cfg->quantum)) return set_error(ITM_ERR_INVALID, "mesh smoothing: the quantum must be finite and above zero");
  if (cfg->flags & ~(uint32_t)ITM_MESH_SMOOTH_PIN_IRREGULAR) return set_error(ITM_ERR_INVALID, "mesh smoothing: unknown flag bits");
  if (cfg->reserved[0] || cfg->reserved[1] || cfg->reserved[2]) return set_error(ITM_ERR_INVALID, "mesh smoothing: reserved words must be 0");
  return ITM_OK;
}

// The call on (vertices, faces, nT, nV > 0): statistics, and for cfg.steps > 0 the smoothed positions in `vertices` and, soup given, the
// soup rewritten through the faces.  A call that cannot get its memory keeps none of it and has written nothing; so has one whose input
// is out of range (ITM_ERR_INVALID).  *written: the launch that writes `vertices` and the soup has been queued and is not known to have
// left at once -- true after success with steps > 0, and after any failure that follows that launch (the positions may have changed:
// the caller marks what depends on them stale); false wherever nothing can have been written.  Synchronises `st`.
static int run_smooth(SmoothBuffers& b, float* vertices, const uint32_t* faces, uint32_t nT, uint32_t nV, float* soup, const itm_mesh_smooth_config& cfg,
                      itm_mesh_smooth_stats* stats, bool* written, hipStream_t st) {
  *written = false;
  if ((size_t)nT * 6 >= 0x7fffffffull || nV >= 0x7fffffffu) return set_error(ITM_ERR_INVALID, "mesh too large to smooth");
  const bool scatter = debug_value(ITM_DEBUG_MESH_SMOOTH_SCATTER) != 0 && cfg.steps > 0;
  const int nChunks = (int)((nV + kSmoothChunk - 1) / kSmoothChunk);
  const uint32_t capHeavy = (uint32_t)std::min<size_t>(nV, (size_t)nT * 6 / kHeavyRow + 1);
  hipError_t e;
  auto fail = [&](hipError_t err, const char* what) {
    b.reset();
    return hip_fail(err, what, __FILE__, __LINE__);
  };
  if ((e = b.rowCount.reserve(nV)) != hipSuccess) return fail(e, "mesh smoothing row counts");
  if ((e = b.rowStart.reserve((size_t)nV + 1)) != hipSuccess) return fail(e, "mesh smoothing row starts");
  if ((e = b.chunkSum.reserve((size_t)nChunks)) != hipSuccess) return fail(e, "mesh smoothing chunk sums");
  if ((e = b.entries.reserve((size_t)nT * 6)) != hipSuccess) return fail(e, "mesh smoothing adjacency rows");
  if ((e = b.heavy.reserve(capHeavy)) != hipSuccess) return fail(e, "mesh smoothing heavy rows");
  if ((e = b.vertexFlags.reserve(nV)) != hipSuccess) return fail(e, "mesh smoothing vertex flags");
  if ((e = b.counters.reserve(kSmoothCounters)) != hipSuccess) return fail(e, "mesh smoothing counters");
  if (cfg.steps > 0) {
    if ((e = b.xa.reserve(nV)) != hipSuccess) return fail(e, "mesh smoothing positions");
    if ((e = b.xb.reserve(nV)) != hipSuccess) return fail(e, "mesh smoothing positions");
    if (scatter && (e = b.sums.reserve((size_t)nV * 4)) != hipSuccess) return fail(e, "mesh smoothing sums");
  }
  const int pin = (cfg.flags & ITM_MESH_SMOOTH_PIN_IRREGULAR) ? 1 : 0;
  ITM_HIP(hipMemsetAsync(b.rowCount, 0, (size_t)nV * 4, st));
  ITM_HIP(hipMemsetAsync(b.counters, 0, kSmoothCounters * 4, st));
  if (nT) smooth_count_kernel<<<grid_for(nT), 256, 0, st>>>(faces, nT, b.rowCount);
  smooth_chunk_sum_kernel<<<nChunks, 256, 0, st>>>(b.rowCount, nV, b.chunkSum);
  smooth_scan_kernel<<<1, 1024, 0, st>>>(b.chunkSum, nChunks, b.rowStart, nV);
  smooth_row_start_kernel<<<nChunks, 256, 0, st>>>(b.rowCount, nV, b.chunkSum, b.rowStart);
  if (nT) smooth_fill_kernel<<<grid_for(nT), 256, 0, st>>>(faces, nT, b.rowStart, b.rowCount, b.entries);
  smooth_topology_kernel<<<(int)std::min<size_t>(grid_for(nV), kTopologyBlocks), 256, 0, st>>>(b.rowStart, b.entries, nV, pin, b.vertexFlags, b.heavy, capHeavy, b.counters);
  smooth_topology_heavy_kernel<<<64, 256, 0, st>>>(b.rowStart, b.entries, pin, b.vertexFlags, b.heavy, capHeavy, b.counters);
  if (cfg.steps > 0) {
    smooth_quantise_kernel<<<grid_for(nV), 256, 0, st>>>(vertices, nV, cfg.quantum, b.xa, b.counters);
    if (scatter) ITM_HIP(hipMemsetAsync(b.sums, 0, (size_t)nV * 32, st));
    int4 *x = b.xa, *xn = b.xb;
    for (uint32_t i = 0; i < cfg.steps; ++i) {
      const int f = (i & 1u) ? cfg.muQ16 : cfg.lambdaQ16;
      if (scatter) {
        if (nT) smooth_scatter_kernel<<<grid_for(nT), 256, 0, st>>>(x, faces, nT, (unsigned long long*)b.sums.get());
        smooth_apply_kernel<<<grid_for(nV), 256, 0, st>>>(x, xn, b.rowStart, b.vertexFlags, nV, f, b.sums);
      } else {
        smooth_gather_kernel<<<grid_for(nV), 256, 0, st>>>(x, xn, b.rowStart, b.entries, b.vertexFlags, nV, f, b.heavy, capHeavy, b.counters);
      }
      std::swap(x, xn);
    }
    *written = true;
    smooth_finish_kernel<<<grid_for(soup ? std::max<size_t>(nV, (size_t)nT * 3) : nV), 256, 0, st>>>(x, b.vertexFlags, nV, cfg.quantum, vertices, faces,
                                                                                                    nT * 3u, soup, b.counters);
  }
  ITM_LAUNCH_CHECK();
  uint32_t counters[kSmoothCounters] = {};
  ITM_HIP(hipMemcpyAsync(counters, b.counters, sizeof(counters), hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (counters[kCountBad]) {                                             // smooth_finish_kernel read the same word and left at once
    *written = false;
    return set_error(ITM_ERR_INVALID, "mesh smoothing: a coordinate is not finite or beyond 2^30 quanta");
  }
  if (counters[kCountHeavy] > capHeavy) return set_error(ITM_ERR_DEVICE, "mesh smoothing: impossible number of long rows");
  if (stats) {
    stats->noVertices = nV; stats->noMoving = counters[kCountMoving]; stats->noIrregular = counters[kCountIrregular];
    stats->noIsolated = counters[kCountIsolated]; stats->maxEntries = counters[kCountMaxEntries]; stats->steps = cfg.steps;
  }
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_smooth_default_config(float voxelSize, itm_mesh_smooth_config* out) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  if (!(voxelSize > 0.0f) || !std::isfinite(voxelSize)) return set_error(ITM_ERR_INVALID, "mesh smoothing: the voxel size must be finite and above zero");
  *out = itm_mesh_smooth_config{};
  out->steps = 20; out->lambdaQ16 = 32768; out->muQ16 = -34734;
  out->quantum = voxelSize / 1024.0f;
  out->flags = ITM_MESH_SMOOTH_PIN_IRREGULAR;
  return ITM_OK;
}

int itm_mesh_smooth(itm_mesh* m, const itm_mesh_smooth_config* cfg, itm_mesh_smooth_stats* stats, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = check_smooth_config(cfg); if (rc) return rc; }
  { const int rc = m->require_index(); if (rc) return rc; }
  if (stats) *stats = itm_mesh_smooth_stats{};
  if (m->noVertices == 0) return ITM_OK;                                 // an empty index: zero statistics, nothing to move
  bool written = false;
  const int rc = run_smooth(m->smooth, m->vertices, m->faces, m->noIndexedTriangles, m->noVertices, m->triangles, *cfg, stats, &written, as_stream(stream));
  if (written) m->vertices_moved();                                      // also when the call failed after the launch that writes the mesh
  if (rc && stats) *stats = itm_mesh_smooth_stats{};
  return rc;
}

int itm_debug_mesh_smooth(const float* vertices_host, uint32_t noVertices, const uint32_t* faces_host, uint32_t noTriangles, const itm_mesh_smooth_config* cfg,
                          float* vertices_out_host, uint8_t* flags_out_host, itm_mesh_smooth_stats* stats, itm_stream stream) {
  if (!stats || (noVertices && (!vertices_host || !vertices_out_host)) || (noTriangles && !faces_host)) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = check_smooth_config(cfg); if (rc) return rc; }
  if ((size_t)noTriangles * 6 >= 0x7fffffffull || noVertices >= 0x7fffffffu) return set_error(ITM_ERR_INVALID, "mesh too large to smooth");
  for (size_t j = 0; j < (size_t)noTriangles * 3; ++j)
    if (faces_host[j] >= noVertices) return set_error(ITM_ERR_INVALID, "a face names a vertex the mesh does not have");
  *stats = itm_mesh_smooth_stats{};
  if (noVertices == 0) return ITM_OK;
  hipStream_t st = as_stream(stream);
  SmoothBuffers b;                    // (freed by its scope)
  DeviceBuffer<float> vertices;
  DeviceBuffer<uint32_t> faces;
  ITM_HIP(vertices.alloc((size_t)noVertices * 3));
  ITM_HIP(faces.alloc((size_t)noTriangles * 3));
  ITM_HIP(hipMemcpyAsync(vertices, vertices_host, (size_t)noVertices * 12, hipMemcpyHostToDevice, st));
  if (noTriangles) ITM_HIP(hipMemcpyAsync(faces, faces_host, (size_t)noTriangles * 12, hipMemcpyHostToDevice, st));
  bool written = false;                                                  // (the hook's arrays are its own: nothing goes stale)
  const int rc = run_smooth(b, vertices, faces, noTriangles, noVertices, nullptr, *cfg, stats, &written, st);
  if (rc) { *stats = itm_mesh_smooth_stats{}; return rc; }
  ITM_HIP(hipMemcpyAsync(vertices_out_host, vertices, (size_t)noVertices * 12, hipMemcpyDeviceToHost, st));
  if (flags_out_host) ITM_HIP(hipMemcpyAsync(flags_out_host, b.vertexFlags, noVertices, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (flags_out_host)
    for (uint32_t k = 0; k < noVertices; ++k) flags_out_host[k] &= (uint8_t)(kIrregular | kIsolated);
  return ITM_OK;
}

}  // extern "C"
