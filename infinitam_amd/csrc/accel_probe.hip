// accel_probe.hip -- read-only test hooks over the acceleration cubes of a hash scene (include/itm_debug.h): what the block directory,
// the slot directory and the sdf mirror hold at given block positions, and a census of everything they hold.  The invariant these
// structures obey (accel_device.h, scene.hip) is kept by eight writers, all through AccelWriter; tests/accel_terms.py restates it on
// the downloaded table and compares it with what these hooks read.  This file is the auditor: it keeps its own address arithmetic, its
// own "absent" values and its own float predicate, and takes from accel_device.h only the constants and cell orders it checks against.
// Nothing here writes scene memory, no product path calls it, and a scene without directories / mirror (or a dense-indexed one)
// reports "nothing".
#include <cstring>

#include "itm_internal.h"

namespace itm {

// what the census counts: [0] directory cells != -1, [1] slot-directory cells != -1, [2] mirror blocks with a cell that is not "absent"
constexpr int kCensusCounts = 3;

// One workgroup per probed position; the 512 mirror values of the block in the block's own order, "absent" where it has no place.
template <bool SHORT>
__global__ void __launch_bounds__(256) accel_probe_kernel(const int32_t* __restrict__ pos, int n, const int32_t* __restrict__ dirPtr, const int32_t* __restrict__ dirSlot,
                                                          const void* __restrict__ mirror, AccelOrigin org, int32_t* __restrict__ cells,
                                                          typename MirrorCodec<SHORT>::T* __restrict__ values) {
  using MC = MirrorCodec<SHORT>;
  const int i = blockIdx.x;
  if (i >= n) return;
  const int bx = pos[3 * i], by = pos[3 * i + 1], bz = pos[3 * i + 2];
  int dirCovered = 0, ptr = -1, slot = -1;
  {
    const uint32_t ux = (uint32_t)(bx - org.dx), uy = (uint32_t)(by - org.dy), uz = (uint32_t)(bz - org.dz);
    if (dirPtr && dir_covers(ux, uy, uz)) {
      const uint32_t cell = dir_cell(ux, uy, uz);
      dirCovered = 1; ptr = dirPtr[cell]; slot = dirSlot ? dirSlot[cell] : -1;
    }
  }
  int mirCovered = 0, page = kPageNone, placed = 0;
  size_t base = 0;
  if (mirror) {
    const uint32_t ux = (uint32_t)(bx - org.mx), uy = (uint32_t)(by - org.my), uz = (uint32_t)(bz - org.mz);
    if (org.mMaxPages < 0) {
      const int bits = mirror_dense_bits(org);
      if (mirror_dense_covers(ux, uy, uz, bits)) { mirCovered = placed = 1; base = (size_t)mirror_dense_cell(ux, uy, uz, bits) << 9; }
    } else if (org.mMaxPages > 0 && mirror_covers(ux, uy, uz)) {
      mirCovered = 1;
      page = org.mTable[mirror_table_index(ux, uy, uz)];
      if (page >= 0 && page < org.mMaxPages) { placed = 1; base = mirror_element(page, mirror_in_page(ux << 3, uy << 3, uz << 3)); }      // (a page index the pool does not have is reported, never followed)
    }
  }
  if (threadIdx.x == 0) {
    int32_t* c = cells + (size_t)i * ITM_ACCEL_PROBE_CELLS;
    c[0] = dirCovered; c[1] = ptr; c[2] = slot; c[3] = mirCovered; c[4] = page; c[5] = placed ? 0 : 1;
  }
  const typename MC::T none = SHORT ? (typename MC::T)-32768 : (typename MC::T)0xffffffffu;
  for (int t = threadIdx.x; t < kBlockVoxels; t += 256)
    values[(size_t)i * kBlockVoxels + t] = placed ? ((const typename MC::T*)mirror)[base + mirror_block_lin((uint32_t)t)] : none;
}

__global__ void __launch_bounds__(256) accel_census_directory_kernel(const int32_t* __restrict__ dirPtr, const int32_t* __restrict__ dirSlot, size_t cells,
                                                                     unsigned long long* __restrict__ counts) {
  unsigned long long a = 0, b = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
    a += dirPtr[i] != -1 ? 1 : 0;
    if (dirSlot) b += dirSlot[i] != -1 ? 1 : 0;
  }
  if (a) atomicAdd(&counts[0], a);
  if (b) atomicAdd(&counts[1], b);
}

// blocks of a kilobyte (short) / two (float bits), whatever order they lie in: a wave per block, eight values per lane
template <bool SHORT>
__global__ void __launch_bounds__(256) accel_census_mirror_kernel(const void* __restrict__ mirror, size_t blocks, unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, waves = ((size_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long dirty = 0;
  for (size_t b = wave; b < blocks; b += waves) {
    bool any;
    if (SHORT) {
      const uint4 v = ((const uint4*)mirror)[b * 64 + lane];
      any = v.x != 0x80008000u || v.y != 0x80008000u || v.z != 0x80008000u || v.w != 0x80008000u;
    } else {
      const uint4 v = ((const uint4*)mirror)[b * 128 + lane], w = ((const uint4*)mirror)[b * 128 + 64 + lane];
      any = (v.x & v.y & v.z & v.w & w.x & w.y & w.z & w.w) != 0xffffffffu;
    }
    if (__ballot(any) != 0ull) ++dirty;
  }
  if (lane == 0 && dirty) atomicAdd(&counts[2], dirty);
}

}  // namespace itm

using namespace itm;

static bool probe_float(const itm_scene* s) { return s->cfg.voxelType == ITM_VOXEL_F || s->cfg.voxelType == ITM_VOXEL_F_RGB; }

extern "C" {

int itm_debug_accel_probe(const itm_scene* s, const int32_t* positions, int n, int32_t* cells, void* values, itm_stream stream) {
  if (!s || n < 0 || (n > 0 && (!positions || !cells || !values))) return set_error(ITM_ERR_INVALID, "accel probe: bad argument");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }      // recorded engine calls are launched first, as for a download
  if (n == 0) return ITM_OK;
  hipStream_t st = as_stream(stream);
  const size_t elem = probe_float(s) ? 4 : 2;
  DeviceBuffer<int32_t> dPos, dCells; DeviceBuffer<void> dValues;      // (freed by their scope)
  hipError_t e = dPos.alloc((size_t)n * 3);
  if (e == hipSuccess) e = dCells.alloc((size_t)n * ITM_ACCEL_PROBE_CELLS);
  if (e == hipSuccess) e = dValues.alloc((size_t)n * kBlockVoxels * elem);
  if (e == hipSuccess) e = hipMemcpyAsync(dPos, positions, (size_t)n * 12, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    if (probe_float(s)) accel_probe_kernel<false><<<n, 256, 0, st>>>(dPos, n, s->dirPtr, s->dirSlot, s->sdfMirror, s->org, dCells, (uint32_t*)dValues.get());
    else accel_probe_kernel<true><<<n, 256, 0, st>>>(dPos, n, s->dirPtr, s->dirSlot, s->sdfMirror, s->org, dCells, (int16_t*)dValues.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(cells, dCells, (size_t)n * ITM_ACCEL_PROBE_CELLS * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(values, dValues, (size_t)n * kBlockVoxels * elem, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "accel probe", __FILE__, __LINE__);
  return ITM_OK;
}

int itm_debug_accel_census(const itm_scene* s, itm_accel_census* out, int32_t* pageTable, itm_stream stream) {
  if (!s || !out) return set_error(ITM_ERR_INVALID, "accel census: null argument");
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  memset(out, 0, sizeof *out);
  if (pageTable) for (size_t i = 0; i < kMirrorTableCells; ++i) pageTable[i] = kPageNone;
  hipStream_t st = as_stream(stream);
  DeviceBuffer<unsigned long long> dCounts;      // (freed by its scope)
  unsigned long long h[kCensusCounts] = {0, 0, 0};
  int32_t pageCounter = 0;
  hipError_t e = dCounts.alloc(kCensusCounts);
  if (e == hipSuccess) e = hipMemsetAsync(dCounts, 0, sizeof h, st);
  if (e == hipSuccess && s->dirPtr) {
    accel_census_directory_kernel<<<4096, 256, 0, st>>>(s->dirPtr, s->dirSlot, kDirCells, dCounts);
    e = hipGetLastError();
  }
  if (e == hipSuccess && s->sdfMirror) {
    const bool paged = s->org.mMaxPages > 0;
    const size_t blocks = paged ? (size_t)s->mirrorPages * kPageBlocks : ((size_t)1 << (3 * mirror_dense_bits(s->org)));
    if (probe_float(s)) accel_census_mirror_kernel<false><<<4096, 256, 0, st>>>(s->sdfMirror, blocks, dCounts);
    else accel_census_mirror_kernel<true><<<4096, 256, 0, st>>>(s->sdfMirror, blocks, dCounts);
    e = hipGetLastError();
    out->mirror_form = paged ? 2 : 1;
    if (e == hipSuccess && paged && pageTable) e = hipMemcpyAsync(pageTable, s->org.mTable, kMirrorTableCells * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && paged) e = hipMemcpyAsync(&pageCounter, s->org.mPages, 4, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, dCounts, sizeof h, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "accel census", __FILE__, __LINE__);
  out->directory_cells = (int64_t)h[0]; out->slot_directory_cells = (int64_t)h[1]; out->mirror_blocks = (int64_t)h[2];
  out->page_counter = pageCounter;
  out->has_directory = s->dirPtr ? 1 : 0;
  return ITM_OK;
}

}  // extern "C"
