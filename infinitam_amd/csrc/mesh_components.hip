// mesh_components.hip -- connected components of the indexed mesh (mesh_index.hip) and the fragment filter built on them.
//
// The reference's ITMMesh is a triangle buffer and nothing else; a TSDF mesh as it leaves marching cubes is one or two surfaces plus a
// cloud of small floating fragments, and every host removes those before it saves a file.  Defined on the present index (include/
// itm_hip.h): vertices are linked iff a triangle names both, a component is a class of the closure, root = its smallest vertex index,
// components numbered by ascending root; per component its vertex and triangle counts and the box of its vertices in the order of
// the IEEE bit patterns.  Integers and order-independent minima only: the result does not depend on the order in which lanes ran.
//
// MI355X design.  Label propagation needs as many rounds as the mesh's graph diameter (hundreds on the test scenes), so the labelling
// is a lock-free union-find on a parent array in HBM:
//   1. components_union_kernel: one lane per triangle joins (a, b) and (a, c).  find_root follows the links and halves the path
//      behind it with atomicCAS(parent[u], p, grandparent); unite links the LARGER of two roots to the smaller one with atomicCAS(
//      parent[a], a, b).  A link always points to a smaller index, so a component's root is its minimum whatever the order.
//      Inside the launch a load of parent[] may be stale: the eight XCDs' L2s are not coherent and an L1 is never refreshed, so the
//      links are read with relaxed agent-scope loads (sc1) and, beyond that, NOTHING rests on a load being fresh: every value ever
//      stored in parent[x] is an ancestor of x, so a stale read only lengthens a walk, and the structure is changed by compare-and-swap
//      alone -- a halving that finds another parent than it read, or a link whose target is no longer a root, changes nothing; the link
//      then carries on from the parent the atomic returned (smaller than the one before: it ends), so no join is ever lost.
//   2. components_compress_kernel (a kernel boundary later: the links are final): parent[k] = root(k).
//   3. components_check_kernel counts the triangles whose corners' roots differ and the vertices whose parent is not a root.  The
//      count travels to the host with the number of components (that read-back sizes the statistics anyway); a non-zero count -- which
//      a correct union never produces: the check is the net, not the algorithm -- runs 1 to 3 again.  The rounds are kept and reported.
//   4. numbering: flags parent[k] == k, ordered compaction (ordered_device.h) -> the roots ascending = the components in order.
//   5. components_stats_kernel: counts and boxes with integer atomics on the component records; the box words hold the monotone
//      unsigned image of the float bits until components_finish_kernel maps them back.  Nearly all triangles belong to one or two
//      components, so the lanes of a wave that share a component aggregate first (one add of the lane count, one min / max per
//      axis from a wave reduction), and a wave keeps those sums in registers over its whole span of consecutive elements while the
//      component stays the same; a mixed wave goes segment by segment.  ITM_DEBUG_MESH_COMPONENTS_PER_LANE: one atomic per lane.
// The work per call does not grow with the diameter: the walks are bounded by tree depth, which the halving keeps short.
//
// itm_mesh_filter_components: keep verdict per component -> keep flag per triangle -> ordered compaction (the kept triangles'
// numbers, ascending) -> the kept triangles gathered into a buffer of the mesh's own and copied back (in place a lane could overwrite
// a triangle before its owner has read it).  pos(t) = kept triangles before t = the lower bound of t in that list, which moves the
// per-block starts of a hash mesh: blockTriangles[b] = pos(min(start, count)); totals = {kept, kept}, so that the last block ends at
// the kept count for the attribute and index paths exactly as after itm_mesh_scene.
#include <algorithm>

#include "itm_internal.h"
#include "mesh_types.h"
#include "ordered_device.h"
#include "wave_utils.h"

namespace itm {


constexpr uint32_t kComponentMaxRounds = 8;       // union rounds before the call gives up (one is what a correct union takes)
constexpr int kComponentWords = 10;               // an itm_mesh_component as uint32 words: root, vertices, triangles, 0, min[3], max[3]
static_assert(sizeof(itm_mesh_component) == kComponentWords * 4, "itm_mesh_component is 40 bytes");

// float bits <-> an unsigned that ascends with the IEEE total order (sign-magnitude: -0.0f just below +0.0f)
__host__ __device__ inline uint32_t order_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ inline uint32_t order_bits(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

// parent[x] inside the union launch: an L2-served load (relaxed, agent scope); possibly stale all the same, which costs steps only
__device__ inline uint32_t link_of(const uint32_t* parent, uint32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a vertex that was read as the root of u's tree; the walk halves the path behind it.  u falls with every step.
__device__ inline uint32_t find_root(uint32_t* parent, uint32_t u) {
  for (;;) {
    const uint32_t p = link_of(parent, u);
    if (p == u) return u;
    const uint32_t g = link_of(parent, p);
    if (g == p) return p;
    atomicCAS(parent + u, p, g);            // only if p is still u's parent: nothing another lane linked is overwritten
    u = g;
  }
}

__device__ inline void unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(parent + a, a, b);   // the larger root takes the smaller as its parent -- if it still is a root
    if (old == a) return;
    a = old;                                 // it was not (linked meanwhile, or read stale): carry on from the parent it has; a + b fell
  }
}

__global__ void __launch_bounds__(256) components_init_kernel(uint32_t* __restrict__ parent, uint32_t nV) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) parent[k] = k;
}

__global__ void __launch_bounds__(256) components_union_kernel(const uint32_t* __restrict__ faces, uint32_t nT, uint32_t* parent) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nT; i += gridDim.x * 256u) {
    const uint32_t a = faces[3 * (size_t)i], b = faces[3 * (size_t)i + 1], c = faces[3 * (size_t)i + 2];
    // two corners with one parent are joined already (whatever was ever stored in parent[x] is an ancestor of x): once the trees are
    // flat that is nearly every edge, settled by three independent loads instead of two walks
    const uint32_t pa = link_of(parent, a), pb = link_of(parent, b), pc = link_of(parent, c);
    if (pa != pb) unite(parent, a, b);
    if (pa != pc && c != b) unite(parent, a, c);
  }
}

// The links are final (the union launch has ended) and lead to a root with parent[r] == r, which this launch never rewrites; the entries
// that other lanes rewrite meanwhile hold an ancestor before and the root after.
__global__ void __launch_bounds__(256) components_compress_kernel(uint32_t* parent, uint32_t nV) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const uint32_t first = parent[k];
    uint32_t r = first;
    for (uint32_t p = parent[r]; p != r; p = parent[r]) r = p;
    if (r != first) parent[k] = r;
  }
}

// counters[2] += triangles whose corners have different roots + vertices whose parent is not a root
__global__ void __launch_bounds__(256) components_check_kernel(const uint32_t* __restrict__ faces, uint32_t nT, const uint32_t* __restrict__ parent, uint32_t nV,
                                                               int32_t* __restrict__ counters) {
  __shared__ int lds[4];
  int bad = 0;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nT; i += gridDim.x * 256u) {
    const uint32_t ra = parent[faces[3 * (size_t)i]], rb = parent[faces[3 * (size_t)i + 1]], rc = parent[faces[3 * (size_t)i + 2]];
    bad += (ra != rb || ra != rc) ? 1 : 0;
  }
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const uint32_t p = parent[k];
    bad += (parent[p] != p) ? 1 : 0;
  }
  const int sum = block_reduce_sum<4>(bad, lds);
  if (threadIdx.x == 0 && sum) atomicAdd(counters + 2, sum);
}

// flags[k] = k is a root, for the nPad = nV rounded up to 8 entries the compaction reads
__global__ void __launch_bounds__(256) components_root_flag_kernel(const uint32_t* __restrict__ parent, uint32_t nV, int nPad, uint8_t* __restrict__ flags,
                                                                   int32_t* __restrict__ chunkCount) {
  flag_chunk(nPad, flags, chunkCount, [&](int k) { return (uint32_t)k < nV && parent[k] == (uint32_t)k; });
}

// component c = the c-th root: its number at the root, its record empty (the box as order keys: min above everything, max below)
__global__ void __launch_bounds__(256) components_number_kernel(const int32_t* __restrict__ roots, uint32_t nC, uint32_t* __restrict__ vertexComponent,
                                                                itm_mesh_component* __restrict__ components) {
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < nC; c += gridDim.x * 256u) {
    const uint32_t root = (uint32_t)roots[c];
    vertexComponent[root] = c;
    uint32_t* w = (uint32_t*)(components + c);
    w[0] = root; w[1] = 0u; w[2] = 0u; w[3] = 0u;
    w[4] = w[5] = w[6] = 0xffffffffu;
    w[7] = w[8] = w[9] = 0u;
  }
}

// reads vertexComponent[] of roots only (written by the launch before), writes it for the others only
__global__ void __launch_bounds__(256) components_spread_kernel(const uint32_t* __restrict__ parent, uint32_t nV, uint32_t* vertexComponent) {
  for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < nV; k += gridDim.x * 256u) {
    const uint32_t p = parent[k];
    if (p != k) vertexComponent[k] = vertexComponent[p];
  }
}

__device__ inline unsigned wave_reduce_umin(unsigned v) { return ~wave_reduce_umax(~v); }

// Adds, for every lane with `valid`, 1 to word `slot` of its component's record and, BOX, its three order keys to the box.  Called by
// all 64 lanes of a wave.  The lanes are taken segment by segment, a segment being the pending lanes that share the component of the
// first pending lane: their count and extrema are reduced over the wave and the segment's first lane issues the atomics.
template <bool BOX>
__device__ inline void add_by_segment(itm_mesh_component* components, bool valid, uint32_t c, int slot, uint32_t kx, uint32_t ky, uint32_t kz) {
  bool pending = valid;
  for (unsigned long long left = __ballot(pending); left != 0ull; left = __ballot(pending)) {      // (uniform: every lane stays in the loop)
    const int leader = __ffsll(left) - 1;
    const uint32_t c0 = (uint32_t)__shfl((int)c, leader);
    const bool mine = pending && c == c0;
    const uint32_t n = (uint32_t)__popcll(__ballot(mine));
    uint32_t lo[3], hi[3];
    if (BOX) {
      lo[0] = wave_reduce_umin(mine ? kx : 0xffffffffu); lo[1] = wave_reduce_umin(mine ? ky : 0xffffffffu); lo[2] = wave_reduce_umin(mine ? kz : 0xffffffffu);
      hi[0] = wave_reduce_umax(mine ? kx : 0u); hi[1] = wave_reduce_umax(mine ? ky : 0u); hi[2] = wave_reduce_umax(mine ? kz : 0u);
    }
    if (lane_id() == leader) {
      uint32_t* w = (uint32_t*)(components + c0);
      atomicAdd(w + slot, n);
      if (BOX) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(w + 4 + a, lo[a]); atomicMax(w + 7 + a, hi[a]); }
      }
    }
    pending = pending && !mine;
  }
}

// A wave's running sums for ONE component, in registers (every member holds the same value in all 64 lanes): as long as whole waves
// of consecutive elements share a component -- nearly always: a mesh is one or two large components, and both vertices and triangles
// are numbered along the buffer -- nothing touches memory; a change of component, a mixed wave (which goes by segment) or the end of
// the wave's span flushes.  So the atomics on the one or two hot records number a few per WAVE OF THE GRID, not per 64 elements.
template <bool BOX>
struct WaveRun {
  static constexpr uint32_t kNone = 0xffffffffu;
  uint32_t c = kNone, n = 0u, lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  __device__ void flush(itm_mesh_component* components, int slot) {
    if (c != kNone && lane_id() == 0) {
      uint32_t* w = (uint32_t*)(components + c);
      atomicAdd(w + slot, n);
      if (BOX) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(w + 4 + a, lo[a]); atomicMax(w + 7 + a, hi[a]); }
      }
    }
    c = kNone; n = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = 0xffffffffu; hi[a] = 0u; }
  }
  // called by all 64 lanes of the wave
  __device__ void add(itm_mesh_component* components, int slot, bool valid, uint32_t ci, uint32_t kx, uint32_t ky, uint32_t kz) {
    const unsigned long long live = __ballot(valid);
    if (live == 0ull) return;
    const uint32_t c0 = (uint32_t)__shfl((int)ci, __ffsll(live) - 1);
    if (__ballot(valid && ci != c0) != 0ull) {            // a mixed wave
      flush(components, slot);
      add_by_segment<BOX>(components, valid, ci, slot, kx, ky, kz);
      return;
    }
    if (c0 != c) { flush(components, slot); c = c0; }
    n += (uint32_t)__popcll(live);
    if (BOX) {
      const uint32_t k[3] = {kx, ky, kz};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint32_t l = wave_reduce_umin(valid ? k[a] : 0xffffffffu), h = wave_reduce_umax(valid ? k[a] : 0u);
        lo[a] = l < lo[a] ? l : lo[a]; hi[a] = h > hi[a] ? h : hi[a];
      }
    }
  }
};

// elements [*begin, *end) of n for this wave: the waves of the grid take consecutive spans, whole multiples of 64
__device__ inline void wave_span(uint32_t n, uint32_t* begin, uint32_t* end) {
  const uint32_t wave = blockIdx.x * (blockDim.x / kWave) + wave_id(), nWaves = gridDim.x * (blockDim.x / kWave);
  const uint32_t span = ((n + nWaves - 1u) / nWaves + 63u) & ~63u;      // wave * span <= n + 64 nWaves: no overflow (n < 2^31)
  *begin = wave * span < n ? wave * span : n;
  *end = n - *begin < span ? n : *begin + span;
}

template <bool PER_LANE, bool BOX>
__device__ inline void vertex_stats(const uint32_t* __restrict__ vertexComponent, const uint32_t* __restrict__ positions, uint32_t nV, itm_mesh_component* components) {
  uint32_t begin, end;
  wave_span(nV, &begin, &end);
  WaveRun<BOX> run;
  for (uint32_t base = begin; base < end; base += kWave) {               // (uniform over the wave: every lane reaches the reductions)
    const uint32_t k = base + lane_id();
    const bool valid = k < end;
    const uint32_t c = valid ? vertexComponent[k] : 0u;
    uint32_t kx = 0u, ky = 0u, kz = 0u;
    if (BOX && valid) { kx = order_key(positions[3 * (size_t)k]); ky = order_key(positions[3 * (size_t)k + 1]); kz = order_key(positions[3 * (size_t)k + 2]); }
    if (PER_LANE) {
      if (!valid) continue;
      uint32_t* w = (uint32_t*)(components + c);
      atomicAdd(w + 1, 1u);
      if (BOX) { atomicMin(w + 4, kx); atomicMin(w + 5, ky); atomicMin(w + 6, kz); atomicMax(w + 7, kx); atomicMax(w + 8, ky); atomicMax(w + 9, kz); }
    } else run.add(components, 1, valid, c, kx, ky, kz);
  }
  run.flush(components, 1);
}

// Vertices: count and box (positions == nullptr: no box).  Triangles: triangleComponent and count.  Integer atomics only.
template <bool PER_LANE>
__global__ void __launch_bounds__(256) components_stats_kernel(const uint32_t* __restrict__ vertexComponent, const uint32_t* __restrict__ positions, uint32_t nV,
                                                               const uint32_t* __restrict__ faces, uint32_t nT, uint32_t* __restrict__ triangleComponent,
                                                               itm_mesh_component* components) {
  if (positions) vertex_stats<PER_LANE, true>(vertexComponent, positions, nV, components);
  else vertex_stats<PER_LANE, false>(vertexComponent, positions, nV, components);
  uint32_t begin, end;
  wave_span(nT, &begin, &end);
  WaveRun<false> run;
  for (uint32_t base = begin; base < end; base += kWave) {
    const uint32_t i = base + lane_id();
    const bool valid = i < end;
    const uint32_t c = valid ? vertexComponent[faces[3 * (size_t)i]] : 0u;
    if (valid) triangleComponent[i] = c;
    if (PER_LANE) {
      if (valid) atomicAdd((uint32_t*)(components + c) + 2, 1u);
    } else run.add(components, 2, valid, c, 0u, 0u, 0u);
  }
  run.flush(components, 2);
}

// the box words back from order keys to float bits; without positions the box is zero
__global__ void __launch_bounds__(256) components_finish_kernel(itm_mesh_component* __restrict__ components, uint32_t nC, int withBox) {
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < nC; c += gridDim.x * 256u) {
    uint32_t* w = (uint32_t*)(components + c);
#pragma unroll
    for (int a = 4; a < kComponentWords; ++a) w[a] = withBox ? order_bits(w[a]) : 0u;
  }
}

// ---- the filter ---------------------------------------------------------------------------------------------------------------------

// keep[c]: in, the host's mask (hasMask); out, the verdict.  counters[3] += components kept
__global__ void __launch_bounds__(256) components_keep_kernel(const itm_mesh_component* __restrict__ components, uint32_t nC, uint32_t minTriangles, int hasMask,
                                                              uint8_t* keep, int32_t* __restrict__ counters) {
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < nC; c += gridDim.x * 256u) {
    const bool k = components[c].noTriangles >= minTriangles && (!hasMask || keep[c] != 0);
    keep[c] = k ? 1 : 0;
    if (k) atomicAdd(counters + 3, 1);
  }
}

__global__ void __launch_bounds__(256) components_triangle_flag_kernel(const uint32_t* __restrict__ triangleComponent, uint32_t nT, int nPad,
                                                                       const uint8_t* __restrict__ keep, uint8_t* __restrict__ flags, int32_t* __restrict__ chunkCount) {
  flag_chunk(nPad, flags, chunkCount, [&](int i) { return (uint32_t)i < nT && keep[triangleComponent[i]] != 0; });
}

// packed[p] = triangle kept[p], p < counters[1]: nine words each
__global__ void __launch_bounds__(256) components_gather_kernel(const uint32_t* __restrict__ triangles, const int32_t* __restrict__ kept, const int32_t* __restrict__ counters,
                                                                uint32_t* __restrict__ packed) {
  const size_t nWords = (size_t)(uint32_t)counters[1] * 9;
  for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < nWords; w += (size_t)gridDim.x * 256) {
    const size_t p = w / 9;
    packed[w] = triangles[(size_t)(uint32_t)kept[p] * 9 + (w - p * 9)];
  }
}

// blockTriangles[b] = kept triangles before block b's old start (cut at the old count): the start of its run in the packed buffer
__global__ void __launch_bounds__(256) components_blocks_kernel(const RenderCounters* __restrict__ lc, int32_t* blockTriangles, int capBlocks, uint32_t count,
                                                                const int32_t* __restrict__ kept, const int32_t* __restrict__ counters) {
  const int nBlocks = lc->noVisibleEntries < capBlocks ? lc->noVisibleEntries : capBlocks;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nBlocks) return;
  uint32_t t0 = (uint32_t)blockTriangles[b];
  t0 = t0 < count ? t0 : count;
  blockTriangles[b] = (int32_t)lower_bound(kept, (uint32_t)counters[1], t0);
}

static int grid_for(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 2048); }
static int padded8(uint32_t n) { return (int)((n + 7u) & ~7u); }

// The labelling of (faces, nT, nV > 0) in `b`; positions: three words per vertex, or nullptr (no box).  A call that cannot get its
// memory keeps none of it.  Synchronises `st`.
static int label_components(ComponentBuffers& b, const uint32_t* faces, uint32_t nT, uint32_t nV, const uint32_t* positions, hipStream_t st,
                            uint32_t* noComponents, uint32_t* rounds) {
  hipError_t e;
  auto fail = [&](hipError_t err, const char* what) {
    b.reset();
    return hip_fail(err, what, __FILE__, __LINE__);
  };
  const int nPad = padded8(nV), nChunks = (nPad + kSweepChunk - 1) / kSweepChunk;
  if ((e = b.parent.reserve(nV)) != hipSuccess) return fail(e, "mesh component links");
  if ((e = b.vertexComponent.reserve(nV)) != hipSuccess) return fail(e, "mesh vertex components");
  if ((e = b.triangleComponent.reserve(nT)) != hipSuccess) return fail(e, "mesh triangle components");
  if ((e = b.flags.reserve((size_t)nPad)) != hipSuccess) return fail(e, "mesh component flags");
  if ((e = b.chunkCount.reserve((size_t)nChunks)) != hipSuccess) return fail(e, "mesh component chunk counts");
  if ((e = b.ids.reserve(nV)) != hipSuccess) return fail(e, "mesh component roots");
  if ((e = b.counters.reserve(4)) != hipSuccess) return fail(e, "mesh component counters");
  components_init_kernel<<<grid_for(nV), 256, 0, st>>>(b.parent, nV);
  int32_t counters[4] = {0, 0, 0, 0};
  uint32_t r = 0;
  do {
    if (r == kComponentMaxRounds) return set_error(ITM_ERR_DEVICE, "mesh components: the union did not settle");
    ITM_HIP(hipMemsetAsync(b.counters, 0, 16, st));
    if (nT) components_union_kernel<<<grid_for(nT), 256, 0, st>>>(faces, nT, b.parent);
    components_compress_kernel<<<grid_for(nV), 256, 0, st>>>(b.parent, nV);
    components_check_kernel<<<grid_for(std::max(nT, nV)), 256, 0, st>>>(faces, nT, b.parent, nV, b.counters);
    components_root_flag_kernel<<<nChunks, 256, 0, st>>>(b.parent, nV, nPad, b.flags, b.chunkCount);
    const int rc = launch_ordered_compaction(b.flags.get(), b.chunkCount, nChunks, nPad, b.ids, (int)nV, b.counters.get(), b.counters + 1, st);
    if (rc) return rc;
    ITM_HIP(hipMemcpyAsync(counters, b.counters, 16, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
    ++r;
  } while (counters[2] != 0);
  const uint32_t nC = (uint32_t)counters[0];
  if (nC == 0 || nC > nV) return set_error(ITM_ERR_DEVICE, "mesh components: impossible component count");
  if ((e = b.components.reserve(nC)) != hipSuccess) return fail(e, "mesh component records");
  components_number_kernel<<<grid_for(nC), 256, 0, st>>>(b.ids, nC, b.vertexComponent, b.components);
  components_spread_kernel<<<grid_for(nV), 256, 0, st>>>(b.parent, nV, b.vertexComponent);
  // a wave per span of consecutive elements, eight waves' worth of them at least: the fewer waves, the fewer flushes onto the hot records
  const int statsGrid = (int)std::min<size_t>(std::max<size_t>(((size_t)std::max(nT, nV) + 2047) / 2048, 1), 256);
  if (debug_value(ITM_DEBUG_MESH_COMPONENTS_PER_LANE))
    components_stats_kernel<true><<<statsGrid, 256, 0, st>>>(b.vertexComponent, positions, nV, faces, nT, b.triangleComponent, b.components);
  else
    components_stats_kernel<false><<<statsGrid, 256, 0, st>>>(b.vertexComponent, positions, nV, faces, nT, b.triangleComponent, b.components);
  components_finish_kernel<<<grid_for(nC), 256, 0, st>>>(b.components, nC, positions ? 1 : 0);
  ITM_LAUNCH_CHECK();
  ITM_HIP(hipStreamSynchronize(st));
  *noComponents = nC;
  *rounds = r;
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_components(itm_mesh* m, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_index(); if (rc) return rc; }
  m->components_recomputing();
  m->noComponents = 0; m->componentRounds = 0;
  if (m->noVertices == 0) { m->components_current(); return ITM_OK; }           // an empty index: no components
  const int rc = label_components(m->comp, m->faces, m->noIndexedTriangles, m->noVertices, (const uint32_t*)m->vertices.get(), as_stream(stream), &m->noComponents,
                                  &m->componentRounds);
  if (rc) { m->noComponents = 0; return rc; }
  m->components_current();
  return ITM_OK;
}

int itm_mesh_components_info(const itm_mesh* m, uint32_t* noComponents, uint32_t* rounds, const uint32_t** vertexComponent_dev,
                             const uint32_t** triangleComponent_dev, const itm_mesh_component** components_dev, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_components(); if (rc) return rc; }
  ITM_HIP(hipStreamSynchronize(as_stream(stream)));
  const bool any = m->noComponents != 0;
  if (noComponents) *noComponents = m->noComponents;
  if (rounds) *rounds = m->componentRounds;
  if (vertexComponent_dev) *vertexComponent_dev = any ? m->comp.vertexComponent.get() : nullptr;
  if (triangleComponent_dev) *triangleComponent_dev = (any && m->noIndexedTriangles) ? m->comp.triangleComponent.get() : nullptr;
  if (components_dev) *components_dev = any ? m->comp.components.get() : nullptr;
  return ITM_OK;
}

int itm_mesh_download_components(const itm_mesh* m, uint32_t* vertexComponent_host, uint32_t capacityVertices, uint32_t* triangleComponent_host,
                                 uint32_t capacityTriangles, itm_mesh_component* components_host, uint32_t capacityComponents, uint32_t* noComponents,
                                 itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_components(); if (rc) return rc; }
  if (noComponents) *noComponents = m->noComponents;
  const bool any = m->noComponents != 0;
  hipStream_t st = as_stream(stream);                                  // (an empty index has no labelling buffers: nothing is copied)
  ITM_HIP(copy_out(vertexComponent_host, m->comp.vertexComponent, any ? m->noVertices : 0u, capacityVertices, 4, st));
  ITM_HIP(copy_out(triangleComponent_host, m->comp.triangleComponent, any ? m->noIndexedTriangles : 0u, capacityTriangles, 4, st));
  ITM_HIP(copy_out(components_host, m->comp.components, m->noComponents, capacityComponents, sizeof(itm_mesh_component), st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

int itm_mesh_filter_components(itm_mesh* m, uint32_t minTriangles, const uint8_t* keep_host, uint32_t noKeep, uint32_t* keptTriangles,
                               uint32_t* keptComponents, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_components(); if (rc) return rc; }
  if (keep_host && noKeep != m->noComponents) return set_error(ITM_ERR_INVALID, "the keep mask needs one entry per component");
  hipStream_t st = as_stream(stream);
  const uint32_t n = m->noIndexedTriangles, nC = m->noComponents;      // the index is current: n is the buffer's count
  if (n == 0) {                                                        // nothing to drop: an empty mesh stays one
    m->soup_rewritten();
    if (keptTriangles) *keptTriangles = 0;
    if (keptComponents) *keptComponents = 0;
    return ITM_OK;
  }
  const int nPad = padded8(n), nChunks = (nPad + kSweepChunk - 1) / kSweepChunk;
  hipError_t e;
  // a filter that cannot get its memory leaves the mesh as it was, labelling included
  if ((e = m->componentKeep.reserve(nC)) != hipSuccess) return hip_fail(e, "mesh component verdicts", __FILE__, __LINE__);
  if ((e = m->packed.reserve((size_t)n * 9)) != hipSuccess) { m->componentKeep.reset(); return hip_fail(e, "mesh packed triangles", __FILE__, __LINE__); }
  if (m->comp.flags.capacity() < (size_t)nPad || m->comp.chunkCount.capacity() < (size_t)nChunks || m->comp.ids.capacity() < n) {
    // the labelling's scratch was sized for the vertices: grow it for the triangles, in buffers of the call's own until all three are had
    DeviceBuffer<uint8_t> flags; DeviceBuffer<int32_t> chunkCount, ids;
    if ((e = flags.alloc((size_t)nPad)) != hipSuccess || (e = chunkCount.alloc((size_t)nChunks)) != hipSuccess || (e = ids.alloc(n)) != hipSuccess) {
      m->componentKeep.reset(); m->packed.reset();
      return hip_fail(e, "mesh filter scratch", __FILE__, __LINE__);
    }
    m->comp.flags = std::move(flags); m->comp.chunkCount = std::move(chunkCount); m->comp.ids = std::move(ids);
  }
  ComponentBuffers& b = m->comp;
  m->soup_rewritten();                                                 // from here on the buffer is being rewritten
  ITM_HIP(hipMemsetAsync(b.counters, 0, 16, st));
  if (keep_host) ITM_HIP(hipMemcpyAsync(m->componentKeep, keep_host, nC, hipMemcpyHostToDevice, st));
  components_keep_kernel<<<grid_for(nC), 256, 0, st>>>(b.components, nC, minTriangles, keep_host ? 1 : 0, m->componentKeep, b.counters);
  components_triangle_flag_kernel<<<nChunks, 256, 0, st>>>(b.triangleComponent, n, nPad, m->componentKeep, b.flags, b.chunkCount);
  const int rc = launch_ordered_compaction(b.flags.get(), b.chunkCount, nChunks, nPad, b.ids, (int)n, b.counters.get(), b.counters + 1, st);
  if (rc) return rc;
  components_gather_kernel<<<grid_for((size_t)n * 9), 256, 0, st>>>((const uint32_t*)m->triangles.get(), b.ids, b.counters, (uint32_t*)m->packed.get());
  if (m->capBlocks > 0)                                                // a hash mesh: the per-block starts follow the triangles
    components_blocks_kernel<<<(m->capBlocks + 255) / 256, 256, 0, st>>>(m->listCounters, m->blockTriangles, m->capBlocks, n, b.ids, b.counters);
  ITM_LAUNCH_CHECK();
  int32_t counters[4] = {0, 0, 0, 0};
  ITM_HIP(hipMemcpyAsync(counters, b.counters, 16, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  const uint32_t kept = (uint32_t)counters[1];
  if (kept > n) return set_error(ITM_ERR_DEVICE, "mesh filter: impossible triangle count");
  if (kept) ITM_HIP(hipMemcpyAsync(m->triangles, m->packed, (size_t)kept * 36, hipMemcpyDeviceToDevice, st));
  // what lies behind the kept triangles is what itm_mesh_scene's cleared buffer holds there (a full buffer's last slot included)
  const uint32_t end = std::min(n + 1u, m->maxTriangles);
  ITM_HIP(hipMemsetAsync(m->triangles + (size_t)kept * 9, 0, (size_t)(end - kept) * 36, st));
  const uint32_t totals[2] = {kept, kept};                             // generated = count: the last block's run ends at the kept count
  ITM_HIP(hipMemcpyAsync(m->totals, totals, 8, hipMemcpyHostToDevice, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (keptTriangles) *keptTriangles = kept;
  if (keptComponents) *keptComponents = (uint32_t)counters[3];
  return ITM_OK;
}

int itm_debug_mesh_components(const uint32_t* faces_host, uint32_t noTriangles, uint32_t noVertices, uint32_t* vertexComponent_host,
                              itm_mesh_component* components_host, uint32_t capComponents, uint32_t* noComponents, uint32_t* rounds, itm_stream stream) {
  if (!noComponents || !rounds || (noTriangles && !faces_host)) return set_error(ITM_ERR_INVALID, "null argument");
  if ((size_t)noTriangles * 3 >= 0x7fffffffull || noVertices >= 0x7fffffffu) return set_error(ITM_ERR_INVALID, "mesh too large to label");
  for (size_t j = 0; j < (size_t)noTriangles * 3; ++j)
    if (faces_host[j] >= noVertices) return set_error(ITM_ERR_INVALID, "a face names a vertex the mesh does not have");
  *noComponents = 0; *rounds = 0;
  if (noVertices == 0) return ITM_OK;
  hipStream_t st = as_stream(stream);
  ComponentBuffers b;               // (freed by its scope)
  DeviceBuffer<uint32_t> faces;
  ITM_HIP(faces.alloc((size_t)noTriangles * 3));
  if (noTriangles) ITM_HIP(hipMemcpyAsync(faces, faces_host, (size_t)noTriangles * 12, hipMemcpyHostToDevice, st));
  const int rc = label_components(b, faces, noTriangles, noVertices, nullptr, st, noComponents, rounds);
  if (rc) return rc;
  ITM_HIP(copy_out(vertexComponent_host, b.vertexComponent, noVertices, noVertices, 4, st));
  ITM_HIP(copy_out(components_host, b.components, *noComponents, capComponents, sizeof(itm_mesh_component), st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

}  // extern "C"
