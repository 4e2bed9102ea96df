// image_maps.hip -- the three colour maps behind ITMMainEngine::GetImage (Engine/ITMMainEngine.cpp:148-160), host loops in the
// reference, kernels here: an image that is only ever looked at never leaves the device to be coloured.
//
// Reference behaviour:
//   DepthToUchar4 / NormalToUchar4 / WeightToUchar4   Engine/ITMVisualisationEngine.cpp:7-107
// The arithmetic follows the reference operation for operation in float32 (no contraction, IEEE division): the output is the
// reference's, byte for byte, wherever its float -> uchar conversion is defined (values in [0, 256)); outside it the conversion
// here saturates and NaN gives 0.  Every output pixel is written: 0 where the reference leaves its cleared image untouched.
//
// Two launches per map, nothing returns to the host:
//   limits   min (and max) of the pixels > 0.  Positive floats order like their bit patterns, so the limits are integer maxima of
//            the bits (the minimum as the maximum of the complement): exact and independent of the order of arrival.  Reduced in
//            the wave (DPP) and the workgroup (LDS), one atomic per workgroup and limit.
//   map      reads the limits where the first launch left them; 4 B in, 4 B out per pixel, float4 loads and 16-byte stores.
// The words that carry the limits belong to the CALL: one slot per (device, stream), from a library-owned pool allocated on first
// use -- calls on one stream are ordered by the stream, calls on two streams never share a slot.  A slot is never re-initialised:
// every call stamps its values with the slot's next epoch in the upper half of the 64-bit word, a stamped value beats every older
// one in the atomic maximum, and a word whose stamp is not the call's means "no pixel > 0".
#include <mutex>
#include <unordered_map>
#include <vector>

#include "itm_internal.h"
#include "wave_utils.h"

namespace itm {

constexpr int kMapThreads = 256;
constexpr int kMapMaxBlocks = 2048;      // grid-stride beyond that

// word 0: epoch << 32 | ~bits(min over the pixels > 0), word 1: epoch << 32 | bits(max over the pixels > 0)
struct ImageLimits { unsigned long long lo, hi; };

// the bits of a valid pixel (v > 0, NaN fails) lie in [1, 0x7f800000], their complements in [0x807fffff, 0xfffffffe]: 0 is
// "nothing seen" for both reductions
__device__ inline void limits_accumulate(float v, uint32_t& loInv, uint32_t& hiBits) {
  if (v > 0.0f) {
    const uint32_t b = __float_as_uint(v);
    loInv = ~b > loInv ? ~b : loInv;
    hiBits = b > hiBits ? b : hiBits;
  }
}

template <bool WANT_MAX>
__global__ void __launch_bounds__(kMapThreads) image_limits_kernel(const float* __restrict__ src, uint32_t n, uint32_t nVec, ImageLimits* __restrict__ lim,
                                                                   uint32_t epoch) {
  __shared__ uint32_t part[2][kMapThreads / kWave];
  uint32_t loInv = 0, hiBits = 0;
  const uint32_t stride = gridDim.x * kMapThreads, first = blockIdx.x * kMapThreads + threadIdx.x;
  const float4* src4 = (const float4*)src;
  for (uint32_t i = first; i < nVec; i += stride) {
    const float4 v = src4[i];
    limits_accumulate(v.x, loInv, hiBits); limits_accumulate(v.y, loInv, hiBits);
    limits_accumulate(v.z, loInv, hiBits); limits_accumulate(v.w, loInv, hiBits);
  }
  for (uint32_t i = nVec * 4 + first; i < n; i += stride) limits_accumulate(src[i], loInv, hiBits);
  loInv = wave_reduce_umax(loInv);
  if (WANT_MAX) hiBits = wave_reduce_umax(hiBits);
  if (lane_id() == 0) { part[0][wave_id()] = loInv; part[1][wave_id()] = hiBits; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < kMapThreads / kWave; ++i) {
      loInv = part[0][i] > loInv ? part[0][i] : loInv;
      hiBits = part[1][i] > hiBits ? part[1][i] : hiBits;
    }
    const unsigned long long stamp = (unsigned long long)epoch << 32;
    if (loInv) {      // (a workgroup that saw a valid pixel has both)
      atomicMax(&lim->lo, stamp | loInv);
      if (WANT_MAX) atomicMax(&lim->hi, stamp | hiBits);
    }
  }
}

// (uchar)x of the reference for x in [0, 256); below: 0, above: 255, NaN: 0 (fmaxf returns the other operand)
__device__ inline uint32_t to_uchar(float x) { return (uint32_t)fminf(fmaxf(x, 0.0f), 255.0f); }
__device__ inline uint32_t pack4(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// interpolate / base, Engine/ITMVisualisationEngine.cpp:7-17: the chain of <= tests in the reference's order (a NaN falls through to 0)
__device__ inline float map_interpolate(float val, float y0, float x0, float y1, float x1) { return (val - x0) * (y1 - y0) / (x1 - x0) + y0; }
__device__ inline float map_base(float val) {
  if (val <= -0.75f) return 0.0f;
  else if (val <= -0.25f) return map_interpolate(val, 0.0f, -0.75f, 1.0f, -0.25f);
  else if (val <= 0.25f) return 1.0f;
  else if (val <= 0.75f) return map_interpolate(val, 1.0f, 0.25f, 0.0f, 0.75f);
  else return 0.0f;
}

struct DepthMap {
  float lo, scale; bool blank;
  __device__ DepthMap(const ImageLimits* lim, uint32_t epoch) {
    // lims[0] = MIN(lims[0], v), lims[1] = MAX(lims[1], v) from (100000, -100000): every v here is > 0
    float l = 100000.0f, h = -100000.0f;
    const unsigned long long a = lim->lo, b = lim->hi;
    if ((uint32_t)(a >> 32) == epoch) {
      const float mn = __uint_as_float(~(uint32_t)a), mx = __uint_as_float((uint32_t)b);
      l = l < mn ? l : mn;
      h = h > mx ? h : mx;
    }
    scale = ((h - l) != 0) ? 1.0f / (h - l) : 1.0f / h;
    lo = l; blank = l == h;
  }
  __device__ uint32_t operator()(float v) const {
    if (blank || !(v > 0.0f)) return 0u;
    const float t = (v - lo) * scale;
    return pack4(to_uchar(map_base(t - 0.5f) * 255.0f), to_uchar(map_base(t) * 255.0f), to_uchar(map_base(t + 0.5f) * 255.0f), 255u);
  }
};

struct WeightMap {
  float m;
  __device__ WeightMap(const ImageLimits* lim, uint32_t epoch) {
    m = 1000.0f;
    const unsigned long long a = lim->lo;
    if ((uint32_t)(a >> 32) == epoch) { const float mn = __uint_as_float(~(uint32_t)a); m = m < mn ? m : mn; }
  }
  __device__ uint32_t operator()(float v) const {
    if (!(v > 0.0f)) return 0u;
    const float s = m / v * 0.8f + 0.2f;
    return pack4(to_uchar((1.0f - s) * 255.0f), to_uchar(s * 255.0f), 0u, 0u);      // alpha stays 0, as in the reference
  }
};

template <class MAP>
__global__ void __launch_bounds__(kMapThreads) image_map_kernel(const float* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n, uint32_t nVec,
                                                                const ImageLimits* __restrict__ lim, uint32_t epoch) {
  const MAP map(lim, epoch);
  const uint32_t stride = gridDim.x * kMapThreads, first = blockIdx.x * kMapThreads + threadIdx.x;
  const float4* src4 = (const float4*)src;
  uint4* dst4 = (uint4*)dst;
  for (uint32_t i = first; i < nVec; i += stride) {
    const float4 v = src4[i];
    dst4[i] = make_uint4(map(v.x), map(v.y), map(v.z), map(v.w));
  }
  for (uint32_t i = nVec * 4 + first; i < n; i += stride) dst[i] = map(src[i]);
}

// NormalToUchar4: one float4 in, one uchar4 out per lane
__global__ void __launch_bounds__(kMapThreads) normal_map_kernel(const float4* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n) {
  const uint32_t stride = gridDim.x * kMapThreads;
  for (uint32_t i = blockIdx.x * kMapThreads + threadIdx.x; i < n; i += stride) {
    const float4 v = src[i];
    uint32_t out = 0u;
    if (v.w >= 0.0f)
      out = pack4(to_uchar((0.3f + (v.x + 1.0f) * 0.35f) * 255.0f), to_uchar((0.3f + (v.y + 1.0f) * 0.35f) * 255.0f),
                  to_uchar((0.3f + (v.z + 1.0f) * 0.35f) * 255.0f), 0u);
    dst[i] = out;
  }
}

// ---- the limits' slots -------------------------------------------------------------------------------------------------------------
// One slot per (device, stream), handed out from blocks of kSlotsPerBlock that are allocated (and zeroed) when the first call on a new
// stream finds none free: no allocation per call after that.  The pool lives as long as the library.
namespace {
constexpr int kSlotsPerBlock = 64;
struct LimitSlot { ImageLimits* words = nullptr; uint32_t epoch = 0; };
struct SlotKey {
  int device; hipStream_t stream;
  bool operator==(const SlotKey& o) const { return device == o.device && stream == o.stream; }
};
struct SlotKeyHash { size_t operator()(const SlotKey& k) const { return std::hash<const void*>()((const void*)k.stream) * 31u + (size_t)k.device; } };
std::mutex g_slotMutex;
std::unordered_map<SlotKey, LimitSlot, SlotKeyHash> g_slots;
struct SlotBlock { int device; DeviceBuffer<ImageLimits> base; int used; };
// lives as long as the process, as the slots always have (never destroyed: no runtime call after the runtime has shut down)
std::vector<SlotBlock>& g_slotBlocks = *new std::vector<SlotBlock>();
}  // namespace

// the slot of stream `st` on the current device, created on first use (the caller holds g_slotMutex); *out is valid on ITM_OK
static int find_slot(hipStream_t st, LimitSlot** out) {
  int device = 0;
  ITM_HIP(hipGetDevice(&device));
  LimitSlot& slot = g_slots[SlotKey{device, st}];
  if (!slot.words) {
    SlotBlock* blk = nullptr;
    for (auto& b : g_slotBlocks) if (b.device == device && b.used < kSlotsPerBlock) { blk = &b; break; }
    if (!blk) {
      DeviceBuffer<ImageLimits> base;
      hipError_t e = base.alloc(kSlotsPerBlock);
      if (e == hipSuccess) e = hipMemset(base, 0, sizeof(ImageLimits) * kSlotsPerBlock);
      if (e == hipSuccess) e = hipDeviceSynchronize();      // once per block: the zeros are in place before any stream uses a slot
      if (e != hipSuccess) { g_slots.erase(SlotKey{device, st}); return hip_fail(e, "image-map limit slots", __FILE__, __LINE__); }
      g_slotBlocks.push_back(SlotBlock{device, std::move(base), 0});
      blk = &g_slotBlocks.back();
    }
    slot.words = blk->base + blk->used++;
  }
  *out = &slot;
  return ITM_OK;
}

// the slot of this call and its epoch; *words / *epoch are valid on ITM_OK
static int acquire_limits(hipStream_t st, ImageLimits** words, uint32_t* epoch) {
  std::lock_guard<std::mutex> lock(g_slotMutex);
  LimitSlot* found = nullptr;
  { const int rc = find_slot(st, &found); if (rc) return rc; }
  LimitSlot& slot = *found;
  if (++slot.epoch == 0) {      // 2^32 calls on this stream: the stamps start over behind a cleared slot
    ITM_HIP(hipMemsetAsync(slot.words, 0, sizeof(ImageLimits), st));
    slot.epoch = 1;
  }
  *words = slot.words; *epoch = slot.epoch;
  return ITM_OK;
}

int image_map_counter(itm_stream stream, const uint32_t* set, uint32_t* get) {
  std::lock_guard<std::mutex> lock(g_slotMutex);
  LimitSlot* slot = nullptr;
  { const int rc = find_slot(as_stream(stream), &slot); if (rc) return rc; }
  if (get) *get = slot->epoch;
  if (set) slot->epoch = *set;
  return ITM_OK;
}

static inline int map_blocks(uint32_t items) {
  const uint32_t b = (items + kMapThreads - 1) / kMapThreads;
  return (int)(b < 1 ? 1 : (b > (uint32_t)kMapMaxBlocks ? (uint32_t)kMapMaxBlocks : b));
}

template <class MAP, bool WANT_MAX>
static int launch_limits_and_map(const float* src, uint8_t* dst, int w, int h, itm_stream stream) {
  if (!src || !dst || w <= 0 || h <= 0 || (unsigned long long)w * (unsigned long long)h > 0x40000000ull) return set_error(ITM_ERR_INVALID, "bad argument");
  if (((uintptr_t)src | (uintptr_t)dst) & 3u) return set_error(ITM_ERR_INVALID, "misaligned image");
  const uint32_t n = (uint32_t)w * (uint32_t)h;
  hipStream_t st = as_stream(stream);
  { const int rc = flush_overlapping(dst, (size_t)n * 4, st); if (rc) return rc; }
  ImageLimits* lim = nullptr; uint32_t epoch = 0;
  { const int rc = acquire_limits(st, &lim, &epoch); if (rc) return rc; }
  // 16-byte accesses where both images allow them; the rest (n % 4 pixels, or everything) one pixel at a time
  const uint32_t nVec = (((uintptr_t)src | (uintptr_t)dst) & 15u) ? 0u : n / 4;
  const int blocks = map_blocks(nVec ? nVec + (n - 4 * nVec) : n);
  image_limits_kernel<WANT_MAX><<<blocks, kMapThreads, 0, st>>>(src, n, nVec, lim, epoch);
  ITM_LAUNCH_CHECK();
  image_map_kernel<MAP><<<blocks, kMapThreads, 0, st>>>(src, (uint32_t*)dst, n, nVec, lim, epoch);
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_depth_to_uchar4(const float* src, uint8_t* dst_rgba, int w, int h, itm_stream stream) {
  return launch_limits_and_map<DepthMap, true>(src, dst_rgba, w, h, stream);
}

int itm_weight_to_uchar4(const float* src, uint8_t* dst_rgba, int w, int h, itm_stream stream) {
  return launch_limits_and_map<WeightMap, false>(src, dst_rgba, w, h, stream);
}

int itm_normal_to_uchar4(const float* src4, uint8_t* dst_rgba, int w, int h, itm_stream stream) {
  if (!src4 || !dst_rgba || w <= 0 || h <= 0 || (unsigned long long)w * (unsigned long long)h > 0x40000000ull) return set_error(ITM_ERR_INVALID, "bad argument");
  if (((uintptr_t)src4 & 15u) || ((uintptr_t)dst_rgba & 3u)) return set_error(ITM_ERR_INVALID, "misaligned image");
  const uint32_t n = (uint32_t)w * (uint32_t)h;
  { const int rc = flush_overlapping(dst_rgba, (size_t)n * 4, as_stream(stream)); if (rc) return rc; }
  normal_map_kernel<<<map_blocks(n), kMapThreads, 0, as_stream(stream)>>>((const float4*)src4, (uint32_t*)dst_rgba, n);
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

}  // extern "C"
