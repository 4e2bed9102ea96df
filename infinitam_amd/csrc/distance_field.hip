// distance_field.hip -- the Euclidean distance transform of a box of the volume (include/itm_hip.h: itm_scene_esdf, itm_esdf_transform):
// one byte of classification per cell, then the squared distance to the nearest site, which site that is, and the signed metric
// distance.  Read-only on the scene; integer arithmetic throughout, so the result equals the sequential definition bit for bit.
//
// Reference behaviour restated: readVoxel (an absent voxel reads TVoxel())   DeviceAgnostic/ITMRepresentationAccess.h:85-142
//                               TVoxel::SDF_valueToFloat                       Utils/ITMLibDefines.h
// The transform itself has no counterpart in the reference.
//
// MI355X design.
//   Classification: one 256-lane workgroup per 8x8x8 tile ALIGNED TO THE SCENE'S BLOCKS (a tile is one block, its halo touches six
//   more), not to the box.  The 3-bit (stored, observed, inside) code of the tile and of the face cells of its one-voxel halo --
//   the surface rule asks for 6-neighbours only, so the halo's edges and corners are not read: 896 voxel reads for 512 cells instead
//   of 3584 -- is staged in LDS through locate_voxel / dense_lin and VX::load (the weight lives in the voxel: the sdf mirror cannot
//   serve this), then every cell derives its SITE bit from LDS.  Cells of the tile outside the box and its halo are not read at all:
//   the coordinate limit of the entry point holds for everything a lane touches.
//   Transform: three passes, x then y then z, each an exact 1-D minimisation of f(q) + (p - q)^2 along its axis, in place on
//   dist2 / nearest: a workgroup stages its panel in LDS, meets one barrier, and only then overwrites the cells it staged -- no
//   other workgroup of the pass reads them.  x pass: a panel is a run of whole lines, contiguous in memory.  y and z passes: a
//   panel is a slab of S adjacent x columns times a whole line, so global loads and stores stay coalesced along x, and the lanes of
//   a wave hold consecutive panel elements: a candidate at offset d is the lane's own element shifted by d * S for every lane --
//   consecutive LDS words, no bank conflicts.  A panel holds about 2048 cells -- S = 8 columns (one 32-byte sector of dist2) for
//   lines of 256 cells and more, up to 64 for short ones -- i.e. 8 KiB of LDS, 16 with `nearest` beside dist2: the 32-wave limit of a
//   CU, not the 160 KiB, bounds the residency (eight workgroups), and the small panels even out the very different scan lengths of
//   the cells (measured on a 256^3 box, unbounded, lean / with nearest: panels of 8192 | 4096 cells 2.33 / 2.37 ms, 4096 | 4096
//   1.53 / 2.11 ms, 2048 | 2048 1.32 / 1.46 ms; profiles/esdf_notes.md).  Lines of 1024 cells take 32 KiB, with `nearest` 4 columns.
//   The scan of a cell walks OUTWARD from it, offsets 0, 1, 2 ... and stops once d^2 exceeds the best value found (f >= 0, so
//   nothing further can win or tie), at the window max_distance, or at the line's last value on either side (first and last
//   position with a value per line, two LDS atomics per staged value): near a surface a cell looks at a handful of candidates and
//   a line without values is not walked at all -- most lines of the x pass (256^3 box, unbounded: 7.0 ms without the per-line
//   range, 2.3 ms with it; profiles/esdf_notes.md).  Equal values go to the smaller position -- which along each axis is the
//   smaller linear index of the site -- so the result is the one of the ascending scan with a strict `<` of the definition.
//   `nearest` is a compile-time variant: the lean kernels neither stage nor track it.
#include "itm_internal.h"
#include "volume_device.h"

namespace itm {

constexpr int kEsdfMaxSide = 1024, kEsdfMaxRadius = 1023;
constexpr long long kEsdfMaxCells = 1ll << 27;
constexpr int kEsdfCoordLimit = 262136;      // query.hip's kPointLimit: block coordinates stay short
constexpr uint32_t kEsdfNone = (uint32_t)ITM_ESDF_NONE;
constexpr int kPanelCells = 2048, kPanelLines = 1024;      // cells and (x pass) lines of a panel

struct EsdfBox { int ox, oy, oz, nx, ny, nz; };

// (stored, observed, inside) of the voxel at p as ITM_ESDF_* bits
template <class VX, bool DENSE>
__device__ inline uint32_t classify_voxel(const VolumeView& vol, int px, int py, int pz, int minWeight, BlockCache& cache) {
  bool stored;
  size_t at;
  if constexpr (DENSE) {
    at = (size_t)dense_lin(vol, px, py, pz, stored);
  } else {
    const long long a = locate_voxel<false>(vol, px, py, pz, cache);
    stored = a >= 0;
    at = stored ? (size_t)a : (size_t)0;
  }
  const typename VX::Reg r = VX::load(vol.vba, at);      // (voxel 0 where none is stored: always a valid address, the value is dropped)
  const bool observed = stored && VX::w_depth(r) >= minWeight;
  const bool inside = observed && VX::to_float(VX::raw_sdf(r)) <= 0.0f;
  return (stored ? (uint32_t)ITM_ESDF_STORED : 0u) | (observed ? (uint32_t)ITM_ESDF_OBSERVED : 0u) | (inside ? (uint32_t)ITM_ESDF_INSIDE : 0u);
}

template <class VX, bool DENSE>
__global__ void __launch_bounds__(256) esdf_classify_kernel(VolumeView vol, EsdfBox box, int sites, int minWeight, uint8_t* __restrict__ state) {
  __shared__ uint8_t code[1000];      // [10][10][10]: the tile and its halo
  // first voxel of the tile: the block of the box's first voxel, plus the workgroup's tile
  const int tx = (((box.ox >> 3) + (int)blockIdx.x) << 3), ty = (((box.oy >> 3) + (int)blockIdx.y) << 3), tz = (((box.oz >> 3) + (int)blockIdx.z) << 3);
  BlockCache cache;
  for (int h = threadIdx.x; h < 1000; h += 256) {
    const int a = h % 10, b = (h / 10) % 10, c = h / 100;
    const int px = tx + a - 1, py = ty + b - 1, pz = tz + c - 1;
    const int onHalo = ((a == 0 || a == 9) ? 1 : 0) + ((b == 0 || b == 9) ? 1 : 0) + ((c == 0 || c == 9) ? 1 : 0);
    // the box with its one-voxel halo, as unsigned: 0 <= p - (o - 1) < n + 2
    const bool near = ((uint32_t)(px - box.ox + 1) < (uint32_t)(box.nx + 2)) & ((uint32_t)(py - box.oy + 1) < (uint32_t)(box.ny + 2)) &
                      ((uint32_t)(pz - box.oz + 1) < (uint32_t)(box.nz + 2));
    uint32_t v = 0u;
    if (near && onHalo <= 1) v = classify_voxel<VX, DENSE>(vol, px, py, pz, minWeight, cache);
    code[h] = (uint8_t)v;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 512; t += 256) {
    const int a = t & 7, b = (t >> 3) & 7, c = t >> 6;
    const uint32_t i = (uint32_t)(tx + a - box.ox), j = (uint32_t)(ty + b - box.oy), k = (uint32_t)(tz + c - box.oz);
    if (i >= (uint32_t)box.nx || j >= (uint32_t)box.ny || k >= (uint32_t)box.nz) continue;
    const int h = (a + 1) + 10 * (b + 1) + 100 * (c + 1);
    const uint32_t me = code[h];
    bool site = false;
    if (me & ITM_ESDF_OBSERVED) {
      if (sites & ITM_ESDF_SITE_SURFACE) {
        const uint32_t flip = me ^ (uint32_t)ITM_ESDF_INSIDE;      // an observed neighbour on the other side: OBSERVED set, INSIDE differs
        const uint32_t want = ITM_ESDF_OBSERVED | ITM_ESDF_INSIDE;
        site = ((code[h - 1] & want) == (flip & want)) | ((code[h + 1] & want) == (flip & want)) | ((code[h - 10] & want) == (flip & want)) |
               ((code[h + 10] & want) == (flip & want)) | ((code[h - 100] & want) == (flip & want)) | ((code[h + 100] & want) == (flip & want));
      }
    } else {
      site = (sites & ITM_ESDF_SITE_UNKNOWN) != 0;
    }
    state[(size_t)i + (size_t)box.nx * ((size_t)j + (size_t)box.ny * (size_t)k)] = (uint8_t)(me | (site ? (uint32_t)ITM_ESDF_SITE : 0u));
  }
}

// One pass of the transform.  AXIS 0: x, reads the SITE bit of `state`; 1: y; 2: z, applies max_distance and writes `distance`.
struct EsdfPass {
  int nx, ny, nz;
  int line;          // cells along the pass's axis
  int group;         // AXIS 0: whole lines per panel; AXIS 1, 2: columns per slab S, a power of two
  int groupShift;    // log2(S)
  int maxOffset;     // the window: min(line - 1, max_distance or line - 1)
  uint32_t limit2;   // max_distance^2, kEsdfNone for "unbounded"
  uint32_t cells;    // nx * ny * nz
  float voxelSize;
};

template <int AXIS, bool NEAREST>
__global__ void __launch_bounds__(256) esdf_pass_kernel(const uint8_t* __restrict__ state, int32_t* dist2, int32_t* nearest, float* __restrict__ distance, EsdfPass p) {
  extern __shared__ uint32_t esdf_lds[];
  const uint32_t L = (uint32_t)p.line;
  const uint32_t lines = (uint32_t)p.group;          // lines of the panel
  const uint32_t panel = lines * L;                  // elements of the panel (AXIS 0: a shorter last panel is cut by `count`)
  uint32_t* lineLo = esdf_lds;                       // per line: first and last position with a value (lo > hi: none)
  uint32_t* lineHi = esdf_lds + lines;
  uint32_t* f = esdf_lds + 2u * lines;
  uint32_t* site = f + panel;                        // NEAREST && AXIS > 0: the site each staged value belongs to
  // element e of the panel: its cell, and its position along the line
  const uint32_t start = (AXIS == 0) ? blockIdx.x * panel : 0u;
  const uint32_t count = (AXIS == 0) ? (p.cells - start < panel ? p.cells - start : panel) : panel;
  const uint32_t step = (AXIS == 0) ? 1u : (uint32_t)p.group;
  const uint32_t col0 = blockIdx.x * (uint32_t)p.group;      // AXIS > 0: first column of the slab
  auto cell_of = [&](uint32_t e, uint32_t& pos, uint32_t& line, bool& valid) -> uint32_t {
    if constexpr (AXIS == 0) {
      line = e / L; pos = e - line * L; valid = true;
      return start + e;
    } else {
      line = e & (step - 1u);
      const uint32_t c = col0 + line;
      pos = e >> p.groupShift;
      valid = c < (uint32_t)p.nx;
      if constexpr (AXIS == 1) return c + (uint32_t)p.nx * (pos + (uint32_t)p.ny * blockIdx.y);
      else return c + (uint32_t)p.nx * (blockIdx.y + (uint32_t)p.ny * pos);
    }
  };
  for (uint32_t l = threadIdx.x; l < lines; l += 256u) { lineLo[l] = L; lineHi[l] = 0u; }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < count; e += 256u) {
    uint32_t pos, line; bool valid;
    const uint32_t g = cell_of(e, pos, line, valid);
    uint32_t v = kEsdfNone;
    if constexpr (AXIS == 0) v = (state[g] & ITM_ESDF_SITE) ? 0u : kEsdfNone;
    else if (valid) v = (uint32_t)dist2[g];
    f[e] = v;
    if constexpr (NEAREST && AXIS > 0) site[e] = valid ? (uint32_t)nearest[g] : 0xffffffffu;
    if (v != kEsdfNone) { atomicMin(&lineLo[line], pos); atomicMax(&lineHi[line], pos); }
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < count; e += 256u) {
    uint32_t pos, line; bool valid;
    const uint32_t g = cell_of(e, pos, line, valid);
    if (!valid) continue;
    // unsigned throughout: kEsdfNone + d^2 does not wrap and never beats a value
    uint32_t best = f[e];
    int at = 0;                                   // offset of the winning candidate
    const int lo = -(int)pos, hi = (int)(L - 1u - pos);
    // no candidate beyond the line's last value on either side: a line without values is not walked at all
    const int first = (int)lineLo[line], last = (int)lineHi[line];
    int reach = first > last ? 0 : ((int)pos - first > last - (int)pos ? (int)pos - first : last - (int)pos);
    if (reach > p.maxOffset) reach = p.maxOffset;
    for (int d = 1; d <= reach && (uint32_t)(d * d) <= best; ++d) {
      const uint32_t dd = (uint32_t)(d * d);
      if (d <= hi) {                              // the larger position first: it wins only when strictly smaller ...
        const uint32_t t = f[e + (uint32_t)d * step] + dd;
        if (t < best) { best = t; if constexpr (NEAREST) at = d; }
      }
      if (-d >= lo) {                             // ... the smaller position also on equality, against everything seen so far
        const uint32_t t = f[e - (uint32_t)d * step] + dd;
        if (t <= best) { best = t; if constexpr (NEAREST) at = -d; }
      }
    }
    if constexpr (AXIS == 2) { if (best > p.limit2) best = kEsdfNone; }
    dist2[g] = (int32_t)best;
    if constexpr (NEAREST) {
      uint32_t n;
      if constexpr (AXIS == 0) n = (uint32_t)((int)g + at);
      else n = site[(uint32_t)((int)e + at * (int)step)];
      nearest[g] = best == kEsdfNone ? -1 : (int32_t)n;
    }
    if constexpr (AXIS == 2) {
      if (distance) {      // (uniform)
        const bool inside = (state[g] & ITM_ESDF_INSIDE) != 0;
        const float m = best == kEsdfNone ? __builtin_inff() : p.voxelSize * sqrtf((float)best);
        distance[g] = inside ? -m : m;
      }
    }
  }
}

static int floor_pow2(int v) { int r = 1; while (r * 2 <= v) r *= 2; return r; }
static int ceil_pow2(int v) { int r = 1; while (r < v) r *= 2; return r; }

template <bool NEAREST>
static void launch_passes(const uint8_t* state, const int32_t size[3], int maxDistance, float voxelSize, int32_t* dist2, int32_t* nearest, float* distance,
                          hipStream_t st) {
  EsdfPass p;
  p.nx = size[0]; p.ny = size[1]; p.nz = size[2];
  p.cells = (uint32_t)((long long)size[0] * size[1] * size[2]);
  p.limit2 = maxDistance > 0 ? (uint32_t)(maxDistance * maxDistance) : kEsdfNone;
  p.voxelSize = voxelSize;
  auto window = [&](int line) { return (maxDistance > 0 && maxDistance < line - 1) ? maxDistance : line - 1; };
  {      // x: whole lines, as many as fill a panel
    p.line = p.nx; p.maxOffset = window(p.nx);
    const long long lines = (long long)p.ny * p.nz;
    long long per = kPanelCells / p.nx;
    if (per > kPanelLines) per = kPanelLines;
    if (per > lines) per = lines;
    p.group = (int)per; p.groupShift = 0;
    const uint32_t grid = (uint32_t)((lines + per - 1) / per);
    esdf_pass_kernel<0, NEAREST><<<grid, 256, (size_t)p.group * (p.line + 2) * 4u, st>>>(state, dist2, nearest, distance, p);
  }
  auto slab = [&](int line) {
    int s = floor_pow2(kPanelCells / line);
    if (s < 8) s = 8;
    if (s > 64) s = 64;
    const int need = ceil_pow2(p.nx);
    if (s > need) s = need;
    auto bytes = [&](int cols) { return (size_t)cols * (line * (NEAREST ? 2 : 1) + 2) * 4u; };
    while (bytes(s) > 65536u) s /= 2;      // (the longest lines with `nearest`: 4 columns)
    p.line = line; p.maxOffset = window(line);
    p.group = s; p.groupShift = __builtin_ctz((unsigned)s);
    return bytes(s);
  };
  {      // y: a slab of columns per plane z
    const size_t lds = slab(p.ny);
    const dim3 grid((uint32_t)((p.nx + p.group - 1) / p.group), (uint32_t)p.nz);
    esdf_pass_kernel<1, NEAREST><<<grid, 256, lds, st>>>(state, dist2, nearest, distance, p);
  }
  {      // z: a slab of columns per row y
    const size_t lds = slab(p.nz);
    const dim3 grid((uint32_t)((p.nx + p.group - 1) / p.group), (uint32_t)p.ny);
    esdf_pass_kernel<2, NEAREST><<<grid, 256, lds, st>>>(state, dist2, nearest, distance, p);
  }
}

static int check_grid(const int32_t size[3], int maxDistance) {
  for (int a = 0; a < 3; ++a)
    if (size[a] < 1 || size[a] > kEsdfMaxSide) return set_error(ITM_ERR_INVALID, "esdf: each side of the box must be in [1, 1024]");
  if ((long long)size[0] * size[1] * size[2] > kEsdfMaxCells) return set_error(ITM_ERR_INVALID, "esdf: the box holds more than 2^27 cells");
  if (maxDistance < 0 || maxDistance > kEsdfMaxRadius) return set_error(ITM_ERR_INVALID, "esdf: max_distance must be in [0, 1023] voxels");
  return ITM_OK;
}

static void transform(const uint8_t* state, const int32_t size[3], int maxDistance, float voxelSize, const itm_esdf_out* out, hipStream_t st) {
  if (out->nearest) launch_passes<true>(state, size, maxDistance, voxelSize, out->dist2, out->nearest, out->distance, st);
  else launch_passes<false>(state, size, maxDistance, voxelSize, out->dist2, nullptr, out->distance, st);
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_esdf_transform(const uint8_t* state_dev, const int32_t size[3], int max_distance, float voxel_size, const itm_esdf_out* out, itm_stream stream) {
  if (!state_dev || !size || !out) return set_error(ITM_ERR_INVALID, "null argument");
  if (!out->dist2) return set_error(ITM_ERR_INVALID, "esdf: dist2 is required (it is the passes' working storage)");
  { const int rc = check_grid(size, max_distance); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  {      // recorded engine calls that read what is written here are launched first (pending.hip)
    const size_t cells = (size_t)size[0] * size[1] * size[2];
    const void* written[3] = {out->dist2, out->nearest, out->distance};
    for (const void* w : written)
      if (w) { const int rc = flush_overlapping(w, cells * 4, st); if (rc) return rc; }
  }
  transform(state_dev, size, max_distance, voxel_size, out, st);
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

int itm_scene_esdf(const itm_scene* s, const itm_esdf_box* box, int sites, int min_weight, int max_distance, const itm_esdf_out* out, itm_stream stream) {
  if (!s || !box || !out) return set_error(ITM_ERR_INVALID, "null argument");
  if (!out->dist2) return set_error(ITM_ERR_INVALID, "esdf: dist2 is required (it is the passes' working storage)");
  if (sites == 0 || (sites & ~(ITM_ESDF_SITE_SURFACE | ITM_ESDF_SITE_UNKNOWN)) != 0)
    return set_error(ITM_ERR_INVALID, "esdf: sites is ITM_ESDF_SITE_SURFACE, ITM_ESDF_SITE_UNKNOWN or both");
  if (min_weight < 1) return set_error(ITM_ERR_INVALID, "esdf: min_weight must be at least 1");
  { const int rc = check_grid(box->size, max_distance); if (rc) return rc; }
  for (int a = 0; a < 3; ++a) {      // the box and its one-voxel halo: o - 1 .. o + n
    const long long lo = (long long)box->origin[a] - 1, hi = (long long)box->origin[a] + box->size[a];
    if (lo <= -(long long)kEsdfCoordLimit || hi >= (long long)kEsdfCoordLimit)
      return set_error(ITM_ERR_INVALID, "esdf: every coordinate of the box and its one-voxel halo must satisfy |p| < 262136");
  }
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const EsdfBox b = {box->origin[0], box->origin[1], box->origin[2], box->size[0], box->size[1], box->size[2]};
  DeviceBuffer<uint8_t> scratch;      // the classification when the caller does not want it (freed on return: the free waits for the launches)
  uint8_t* state = out->state;
  if (!state) {
    ITM_HIP(scratch.alloc((size_t)b.nx * b.ny * b.nz));
    state = scratch;
  }
  const VolumeView vol = make_volume(s);
  const dim3 grid((uint32_t)(((b.ox + b.nx - 1) >> 3) - (b.ox >> 3) + 1), (uint32_t)(((b.oy + b.ny - 1) >> 3) - (b.oy >> 3) + 1),
                  (uint32_t)(((b.oz + b.nz - 1) >> 3) - (b.oz >> 3) + 1));
  const int rc = dispatch_volume(s, [&](auto vx, auto dense) {
    esdf_classify_kernel<decltype(vx), dense.value><<<grid, 256, 0, st>>>(vol, b, sites, min_weight, state);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  transform(state, box->size, max_distance, s->prm.voxelSize, out, st);
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // extern "C"
