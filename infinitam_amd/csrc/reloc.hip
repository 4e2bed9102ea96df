// reloc.hip -- keyframe relocaliser (include/itm_hip.h: itm_reloc_*): randomised fern codes of a small, smoothed depth image
// (Glocker et al., "Real-Time RGB-D Camera Relocalization via Randomized Ferns for Keyframe Encoding"), a database of keyframe
// codes in HBM with their poses on the host, and the nearest-code search.  The reference at this revision has no relocaliser; the
// sequential definition in the header is the specification and tests/reloc_terms.py its restatement.
//
// MI355X design.
//   image    FilterSubsampleWithHoles per level through itm_filter_subsample_with_holes (the tracker's kernel), then two launches of
//            blur_kernel (rows, then columns), one lane per pixel: ~1 200 pixels, a launch each -- edges and holes, not speed.
//   code     one lane per fern, one byte each, into a row padded with zeros to a multiple of 16 bytes.
//   search   a streaming read of count x rowBytes.  A row is rowBytes / 16 vectors of 16 bytes; a GROUP of L lanes (L: the power of
//            two >= that number) owns a row, a wave therefore 64 / L rows per pass, 64 x 16 contiguous bytes when the row fills its
//            group (the default 500 ferns: 512 bytes, L = 32).  Every lane keeps ITS 16 bytes of the query in registers (staged once
//            per workgroup through LDS), so a pass is one load, four XORs, the exact zero-byte test on each word, ONE popcount, and
//            log2(L) cross-lane adds.  Four passes are in flight per lane.  The group's first lane forms the key
//            sim << 32 | (0xFFFFFFFF - id) and keeps its eight largest in registers (a wave-uniform test skips the insertion once no
//            lane's key beats its eighth); the maximum over keys is the defined order whatever the arrival order.  A workgroup ends
//            by extracting its eight largest keys (wave maxima, then the four waves' through LDS) into partial[8 * blockIdx.x];
//            the second launch, one workgroup, does the same over the partials and writes ids and distances into the pinned record.
//            No cross-workgroup ordering anywhere: two launches on one stream.
//   harvest  decided on the host from the pinned record after the call's one synchronise; the row is then copied device to device
//            on the same stream (nothing waits for it).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "itm_internal.h"

namespace itm {

constexpr int kRelocMaxK = ITM_RELOC_MAX_K;
constexpr int kSearchGridCap = 1024;      // workgroups of the scan (4 per CU); the rest is grid-stride
constexpr int kSearchUnroll = 4;          // passes in flight per lane

struct RelocTaps { float t[9]; };

// the pinned result record of one search
struct RelocRecord { int32_t ids[kRelocMaxK]; float dist[kRelocMaxK]; };

// one pass of the hole-aware separable blur: along x (dx = 1, dy = 0) or along y
__global__ void __launch_bounds__(256) reloc_blur_kernel(const float* __restrict__ in, float* __restrict__ out, int w, int h, int R, RelocTaps taps, int alongY) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  const int x = i % w, y = i / w;
  float s = 0.0f, n = 0.0f;
  for (int k = -R; k <= R; ++k) {
    const int px = alongY ? x : x + k, py = alongY ? y + k : y;
    if (px < 0 || py < 0 || px >= w || py >= h) continue;
    const float v = in[px + py * w];
    const float t = taps.t[k < 0 ? -k : k];
    if (v > 0.0f) { s = s + t * v; n = n + t; }
  }
  out[i] = n > 0.0f ? s / n : 0.0f;
}

__global__ void __launch_bounds__(256) reloc_code_kernel(const float* __restrict__ img, const int32_t* __restrict__ pixel, const float* __restrict__ threshold,
                                                         int F, int D, uint8_t* __restrict__ code) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  uint32_t c = 0;
  for (int d = 0; d < D; ++d) c |= (img[pixel[f * D + d]] > threshold[f * D + d]) ? (1u << d) : 0u;
  code[f] = (uint8_t)c;
}

// bit 7 of every byte of x that is zero (exact: no carries between bytes)
__device__ inline uint32_t zero_bytes(uint32_t x) {
  const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  return ~(t | x | 0x7F7F7F7Fu);
}

__device__ inline int equal_bytes(const uint4& a, const uint4& b) {
  const uint32_t m = zero_bytes(a.x ^ b.x) | (zero_bytes(a.y ^ b.y) >> 1) | (zero_bytes(a.z ^ b.z) >> 2) | (zero_bytes(a.w ^ b.w) >> 3);
  return __popc(m);
}

// the eight largest keys a lane has seen, descending; 0 = none (a key of a row is >= 1)
struct TopKeys {
  unsigned long long t[kRelocMaxK];
  __device__ void clear() {
#pragma unroll
    for (int j = 0; j < kRelocMaxK; ++j) t[j] = 0ull;
  }
  __device__ void insert(unsigned long long key) {
#pragma unroll
    for (int j = 0; j < kRelocMaxK; ++j) {
      const bool up = key > t[j];
      const unsigned long long lo = up ? t[j] : key;
      t[j] = up ? key : t[j];
      key = lo;
    }
  }
  __device__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < kRelocMaxK; ++j) t[j] = t[j + 1];
    t[kRelocMaxK - 1] = 0ull;
  }
};

__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// The wave's eight largest keys, descending: out[j] the same in every lane.  Keys of rows are distinct (the id is part of the key),
// so exactly one lane owns a non-zero maximum and gives it up.
__device__ inline void wave_extract(TopKeys& mine, unsigned long long out[kRelocMaxK]) {
#pragma unroll
  for (int j = 0; j < kRelocMaxK; ++j) {
    const unsigned long long m = wave_max_u64(mine.t[0]);
    out[j] = m;
    if (m != 0ull && mine.t[0] == m) mine.pop();
  }
}

// A workgroup's (256 lanes) eight largest keys into dst[0 .. 8): the waves' through LDS, then wave 0's extraction over the 32
__device__ inline void block_extract(TopKeys& mine, unsigned long long* lds /* [32] */, unsigned long long* __restrict__ dst) {
  unsigned long long best[kRelocMaxK];
  wave_extract(mine, best);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kRelocMaxK; ++j) lds[wave * kRelocMaxK + j] = best[j];
  }
  __syncthreads();
  if (wave == 0) {
    TopKeys one;
    one.clear();
    one.t[0] = lane < 4 * kRelocMaxK ? lds[lane] : 0ull;
    wave_extract(one, best);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < kRelocMaxK; ++j) dst[j] = best[j];
    }
  }
}

// The scan.  rowVec: 16-byte vectors per row; LOG_L: log2 of the lanes that own a row; pad: the zero bytes at the end of every row
// (they equal the query's and are taken off the count).  Rows past `count` are read at row 0 and dropped.
template <int LOG_L>
__global__ void __launch_bounds__(256) reloc_scan_kernel(const uint4* __restrict__ db, const uint4* __restrict__ query, uint32_t count, int rowVec, int pad,
                                                         unsigned long long* __restrict__ partial) {
  constexpr int L = 1 << LOG_L, ROWS = 64 / L;      // rows per wave and pass
  __shared__ uint4 q_lds[64];
  __shared__ unsigned long long keys_lds[4 * kRelocMaxK];
  if (threadIdx.x < 64) q_lds[threadIdx.x] = (int)threadIdx.x < rowVec ? query[threadIdx.x] : make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const int lane = threadIdx.x & 63, sub = lane & (L - 1), rowInWave = lane >> LOG_L;
  const bool loads = sub < rowVec;
  const uint4 q = q_lds[sub];
  TopKeys top;
  top.clear();
  const uint32_t waves = gridDim.x * 4u, gw = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t passes = (count + (uint32_t)ROWS - 1u) / (uint32_t)ROWS;
  for (uint32_t base = 0; base < passes; base += waves * (uint32_t)kSearchUnroll) {      // (uniform over the grid)
    uint4 v[kSearchUnroll];
    uint32_t row[kSearchUnroll];
#pragma unroll
    for (int u = 0; u < kSearchUnroll; ++u) {
      row[u] = (base + (uint32_t)u * waves + gw) * (uint32_t)ROWS + (uint32_t)rowInWave;
      const size_t at = (row[u] < count && loads) ? (size_t)row[u] * (size_t)rowVec + (size_t)sub : (size_t)0;
      v[u] = db[at];
    }
#pragma unroll
    for (int u = 0; u < kSearchUnroll; ++u) {
      int eq = loads ? equal_bytes(v[u], q) : 0;
#pragma unroll
      for (int off = L >> 1; off >= 1; off >>= 1) eq += __shfl_xor(eq, off, 64);
      const bool mine = sub == 0 && row[u] < count;
      const unsigned long long key = mine ? ((unsigned long long)(uint32_t)(eq - pad) << 32) | (unsigned long long)(0xFFFFFFFFu - row[u]) : 0ull;
      if (__any(key > top.t[kRelocMaxK - 1])) top.insert(key);      // (uniform) a key that enters no lane's list changes nothing
    }
  }
  block_extract(top, keys_lds, partial + (size_t)blockIdx.x * kRelocMaxK);
}

// The second launch: one workgroup over the scan's partial keys; ids and distances into the record.
__global__ void __launch_bounds__(256) reloc_merge_kernel(const unsigned long long* __restrict__ partial, int nPartial, int F, int k, RelocRecord* __restrict__ rec) {
  __shared__ unsigned long long keys_lds[4 * kRelocMaxK + kRelocMaxK];
  TopKeys top;
  top.clear();
  for (int i = threadIdx.x; i < nPartial; i += 256) top.insert(partial[i]);
  block_extract(top, keys_lds, keys_lds + 4 * kRelocMaxK);
  __syncthreads();
  if (threadIdx.x < kRelocMaxK) {
    const int j = threadIdx.x;
    const unsigned long long key = keys_lds[4 * kRelocMaxK + j];
    const bool have = j < k && key != 0ull;
    const int sim = (int)(uint32_t)(key >> 32);
    rec->ids[j] = have ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    rec->dist[j] = have ? (float)(F - sim) / (float)F : 1.0f;
  }
}

static int log2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

}  // namespace itm

using namespace itm;

struct itm_reloc {
  itm_reloc_config cfg;
  int ws = 0, hs = 0;             // the small image
  int rowBytes = 0;               // numFerns rounded up to 16
  int count = 0;
  std::vector<int32_t> pixelHost;
  std::vector<float> thresholdHost;
  std::vector<float> poses;       // 16 per row
  // device
  std::vector<itm::DeviceBuffer<float>> pyramid;     // I_1 .. I_levels
  itm::DeviceBuffer<float> blurTmp, blurOut;         // ws x hs each
  const float* image = nullptr;   // S of the last encode: blurOut, the last pyramid level or (levels = 0, R = 0) a copy in blurOut
  itm::DeviceBuffer<int32_t> pixel;
  itm::DeviceBuffer<float> threshold;
  itm::DeviceBuffer<uint8_t> code, query;            // rowBytes each, zero beyond numFerns
  itm::DeviceBuffer<uint8_t> db;  // capacity x rowBytes
  itm::DeviceBuffer<unsigned long long> partial;     // kSearchGridCap x 8
  itm::PinnedBuffer<uint8_t> queryPinned;            // rowBytes: a caller's code on its way to `query`
  itm::PinnedBuffer<RelocRecord> rec;                // pinned, mapped
  hipStream_t last = nullptr;     // the stream of the last enqueueing call: the host-side calls wait for it
  bool used = false;              // `last` is one
  hipEvent_t ev[2] = {nullptr, nullptr};             // itm_debug_reloc_search_ms: around the search's launches
  bool timing = false, timed = false;
  bool encoded = false;
};

namespace {

void reloc_free(itm_reloc* r) {
  if (!r) return;
  for (hipEvent_t e : r->ev) if (e) (void)hipEventDestroy(e);
  delete r;
}

// what is wrong with a configuration, or nullptr
const char* config_fault(const itm_reloc_config* c) {
  if (c->w < 1 || c->h < 1 || c->levels < 0 || c->levels > 30) return "reloc: image size or levels out of range";
  if ((c->w >> c->levels) < 1 || (c->h >> c->levels) < 1) return "reloc: the image size does not survive `levels` halvings";
  if (c->blurRadius < 0 || c->blurRadius > 8) return "reloc: blurRadius outside 0..8";
  if (c->numFerns < 1 || c->numFerns > ITM_RELOC_MAX_FERNS) return "reloc: numFerns outside 1..1024";
  if (c->numDecisions < 1 || c->numDecisions > 8) return "reloc: numDecisions outside 1..8";
  if (c->capacity < 1) return "reloc: capacity < 1";
  return nullptr;
}

// A call that enqueues on `st`: what an earlier call left on another stream is waited for first (a host that stays on one stream
// never waits here).
int enter_reloc(itm_reloc* r, hipStream_t st) {
  if (r->used && r->last != st) ITM_HIP(hipStreamSynchronize(r->last));
  r->last = st; r->used = true;
  return ITM_OK;
}

int wait_reloc(itm_reloc* r) {
  if (r->used) ITM_HIP(hipStreamSynchronize(r->last));
  return ITM_OK;
}

int launch_scan(itm_reloc* r, const uint8_t* query, int k, hipStream_t st) {
  const int rowVec = r->rowBytes / 16, logL = log2_ceil(rowVec), rows = 64 >> logL;
  int grid = 0;
  if (r->timing) ITM_HIP(hipEventRecord(r->ev[0], st));
  if (r->count > 0) {
    const long long passes = ((long long)r->count + rows - 1) / rows;
    const long long wgs = (passes + 4 * kSearchUnroll - 1) / (4 * kSearchUnroll);
    grid = (int)(wgs < kSearchGridCap ? wgs : kSearchGridCap);
    const int pad = r->rowBytes - r->cfg.numFerns;
#define ITM_SCAN(LL) case LL: reloc_scan_kernel<LL><<<grid, 256, 0, st>>>((const uint4*)r->db.get(), (const uint4*)query, (uint32_t)r->count, rowVec, pad, r->partial); break;
    switch (logL) { ITM_SCAN(0) ITM_SCAN(1) ITM_SCAN(2) ITM_SCAN(3) ITM_SCAN(4) ITM_SCAN(5) ITM_SCAN(6) }
#undef ITM_SCAN
    ITM_LAUNCH_CHECK();
  }
  reloc_merge_kernel<<<1, 256, 0, st>>>(r->partial, grid * kRelocMaxK, r->cfg.numFerns, k, r->rec.device());
  ITM_LAUNCH_CHECK();
  if (r->timing) { ITM_HIP(hipEventRecord(r->ev[1], st)); r->timed = true; }
  return ITM_OK;
}

int check_k(int k, const int32_t* ids, const float* dist) {
  if (k < 1 || k > ITM_RELOC_MAX_K) return set_error(ITM_ERR_INVALID, "reloc: k outside 1..ITM_RELOC_MAX_K");
  if (!ids || !dist) return set_error(ITM_ERR_INVALID, "null argument");
  return ITM_OK;
}

const char kRelocFile[] = "/relocaliser.dat";
const uint32_t kRelocMagic = 0x4C52544Du;      // "MTRL"

}  // namespace

extern "C" {

int itm_reloc_default_config(int w, int h, itm_reloc_config* cfg) {
  if (!cfg || w < 1 || h < 1) return set_error(ITM_ERR_INVALID, "reloc: bad argument");
  memset(cfg, 0, sizeof *cfg);
  cfg->w = w; cfg->h = h;
  int L = 0;
  while ((w >> L) > 40) ++L;
  if ((h >> L) < 1) return set_error(ITM_ERR_INVALID, "reloc: the image size does not survive the default levels");
  cfg->levels = L;
  cfg->blurRadius = 6;
  for (int i = 0; i <= 6; ++i) cfg->blurTaps[i] = (float)exp(-(double)(i * i) / (2 * 2.5 * 2.5));
  cfg->numFerns = 500; cfg->numDecisions = 4; cfg->capacity = 65536;
  return ITM_OK;
}

int itm_reloc_default_ferns(const itm_reloc_config* cfg, uint64_t seed, float lo, float hi, int32_t* pixel, float* threshold) {
  if (!cfg || !pixel || !threshold) return set_error(ITM_ERR_INVALID, "null argument");
  if (const char* why = config_fault(cfg)) return set_error(ITM_ERR_INVALID, why);
  const uint64_t npix = (uint64_t)(cfg->w >> cfg->levels) * (uint64_t)(cfg->h >> cfg->levels);
  uint64_t x = seed;
  auto next = [&x]() {      // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  const int n = cfg->numFerns * cfg->numDecisions;
  for (int i = 0; i < n; ++i) {
    pixel[i] = (int32_t)((next() >> 32) % npix);
    const float u = (float)(next() >> 40) * (1.0f / 16777216.0f);
    threshold[i] = lo + (hi - lo) * u;
  }
  return ITM_OK;
}

int itm_reloc_create(const itm_reloc_config* cfg, const int32_t* pixel_host, const float* threshold_host, itm_reloc** out) {
  if (!cfg || !pixel_host || !threshold_host || !out) return set_error(ITM_ERR_INVALID, "null argument");
  if (const char* why = config_fault(cfg)) return set_error(ITM_ERR_INVALID, why);
  const int ws = cfg->w >> cfg->levels, hs = cfg->h >> cfg->levels, n = cfg->numFerns * cfg->numDecisions;
  for (int i = 0; i < n; ++i)
    if (pixel_host[i] < 0 || pixel_host[i] >= ws * hs) return set_error(ITM_ERR_INVALID, "reloc: a fern's pixel index lies outside the small image");
  itm_reloc* r = new (std::nothrow) itm_reloc();
  if (!r) return set_error(ITM_ERR_DEVICE, "out of host memory");
  r->cfg = *cfg; r->ws = ws; r->hs = hs;
  r->rowBytes = (cfg->numFerns + 15) & ~15;
  r->pixelHost.assign(pixel_host, pixel_host + n);
  r->thresholdHost.assign(threshold_host, threshold_host + n);
  hipError_t e = hipSuccess;
  auto dev = [&e](auto& buf, size_t elems) { if (e == hipSuccess) e = buf.alloc(elems, 1); };
  r->pyramid.resize((size_t)cfg->levels);
  for (int l = 1; l <= cfg->levels; ++l) dev(r->pyramid[(size_t)l - 1], (size_t)(cfg->w >> l) * (size_t)(cfg->h >> l));
  dev(r->blurTmp, (size_t)ws * hs); dev(r->blurOut, (size_t)ws * hs);
  dev(r->pixel, (size_t)n); dev(r->threshold, (size_t)n);
  dev(r->code, (size_t)r->rowBytes); dev(r->query, (size_t)r->rowBytes);
  dev(r->db, (size_t)cfg->capacity * (size_t)r->rowBytes);
  dev(r->partial, (size_t)kSearchGridCap * kRelocMaxK);
  if (e == hipSuccess) e = r->queryPinned.alloc((size_t)r->rowBytes, hipHostMallocDefault);
  if (e == hipSuccess) e = r->rec.alloc(1, hipHostMallocMapped | hipHostMallocCoherent, true);
  if (e == hipSuccess) e = hipMemcpy(r->pixel, pixel_host, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(r->threshold, threshold_host, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(r->code, 0, (size_t)r->rowBytes);
  if (e == hipSuccess) e = hipMemset(r->query, 0, (size_t)r->rowBytes);
  if (e == hipSuccess) e = hipMemset(r->blurOut, 0, (size_t)ws * hs * 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { reloc_free(r); return hip_fail(e, "itm_reloc_create", __FILE__, __LINE__); }
  r->image = r->blurOut;
  *out = r;
  return ITM_OK;
}

int itm_reloc_destroy(itm_reloc* r) {
  if (r) (void)wait_reloc(r);
  reloc_free(r);
  return ITM_OK;
}

int itm_reloc_encode(itm_reloc* r, const float* depth_dev, itm_stream stream) {
  if (!r || !depth_dev) return set_error(ITM_ERR_INVALID, "null argument");
  hipStream_t st = as_stream(stream);
  { const int rc = enter_reloc(r, st); if (rc) return rc; }
  const float* cur = depth_dev;
  for (int l = 1; l <= r->cfg.levels; ++l) {
    const int rc = itm_filter_subsample_with_holes(cur, r->cfg.w >> (l - 1), r->cfg.h >> (l - 1), r->pyramid[(size_t)l - 1], stream);
    if (rc) return rc;
    cur = r->pyramid[(size_t)l - 1];
  }
  const int P = r->ws * r->hs, grid = (P + 255) / 256;
  if (r->cfg.blurRadius > 0) {
    RelocTaps taps;
    memcpy(taps.t, r->cfg.blurTaps, sizeof taps.t);
    reloc_blur_kernel<<<grid, 256, 0, st>>>(cur, r->blurTmp, r->ws, r->hs, r->cfg.blurRadius, taps, 0);
    reloc_blur_kernel<<<grid, 256, 0, st>>>(r->blurTmp, r->blurOut, r->ws, r->hs, r->cfg.blurRadius, taps, 1);
    ITM_LAUNCH_CHECK();
    cur = r->blurOut;
  } else if (r->cfg.levels == 0) {      // the caller's image may change before the code is read back: keep what was encoded
    ITM_HIP(hipMemcpyAsync(r->blurOut, depth_dev, (size_t)P * 4, hipMemcpyDeviceToDevice, st));
    cur = r->blurOut;
  }
  r->image = cur;
  reloc_code_kernel<<<(r->cfg.numFerns + 255) / 256, 256, 0, st>>>(cur, r->pixel, r->threshold, r->cfg.numFerns, r->cfg.numDecisions, r->code);
  ITM_LAUNCH_CHECK();
  r->encoded = true;
  return ITM_OK;
}

int itm_reloc_find(itm_reloc* r, const uint8_t* code_host, int k, int32_t* ids_host, float* dist_host, itm_stream stream) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = check_k(k, ids_host, dist_host); if (rc) return rc; }
  if (!code_host && !r->encoded) return set_error(ITM_ERR_INVALID, "reloc: no code has been encoded yet");
  hipStream_t st = as_stream(stream);
  { const int rc = enter_reloc(r, st); if (rc) return rc; }
  const uint8_t* q = r->code;
  if (code_host) {
    memset(r->queryPinned, 0, (size_t)r->rowBytes);
    memcpy(r->queryPinned, code_host, (size_t)r->cfg.numFerns);
    ITM_HIP(hipMemcpyAsync(r->query, r->queryPinned, (size_t)r->rowBytes, hipMemcpyHostToDevice, st));
    q = r->query;
  }
  { const int rc = launch_scan(r, q, k, st); if (rc) return rc; }
  ITM_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < k; ++j) { ids_host[j] = r->rec->ids[j]; dist_host[j] = r->rec->dist[j]; }
  return ITM_OK;
}

int itm_reloc_process_frame(itm_reloc* r, const float* depth_dev, const float M_d[16], int harvest, float harvestThreshold, int k, int32_t* ids_host,
                            float* dist_host, int32_t* added, itm_stream stream) {
  if (!r || !depth_dev || !added || (harvest && !M_d)) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = check_k(k, ids_host, dist_host); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  { const int rc = itm_reloc_encode(r, depth_dev, stream); if (rc) return rc; }
  { const int rc = launch_scan(r, r->code, k, st); if (rc) return rc; }
  ITM_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < k; ++j) { ids_host[j] = r->rec->ids[j]; dist_host[j] = r->rec->dist[j]; }
  *added = -1;
  if (harvest && (r->count == 0 || r->rec->dist[0] > harvestThreshold)) {
    if (r->count >= r->cfg.capacity) { *added = -2; return ITM_OK; }
    ITM_HIP(hipMemcpyAsync(r->db + (size_t)r->count * (size_t)r->rowBytes, r->code, (size_t)r->rowBytes, hipMemcpyDeviceToDevice, st));
    r->poses.insert(r->poses.end(), M_d, M_d + 16);
    *added = r->count++;
  }
  return ITM_OK;
}

int itm_reloc_info(const itm_reloc* r, int32_t* count, itm_reloc_config* cfg) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  if (count) *count = r->count;
  if (cfg) *cfg = r->cfg;
  return ITM_OK;
}

int itm_reloc_get_pose(const itm_reloc* r, int32_t id, float M[16]) {
  if (!r || !M) return set_error(ITM_ERR_INVALID, "null argument");
  if (id < 0 || id >= r->count) return set_error(ITM_ERR_INVALID, "reloc: id outside the database");
  memcpy(M, r->poses.data() + (size_t)id * 16, 64);
  return ITM_OK;
}

int itm_debug_reloc_search_ms(itm_reloc* r, int enable, float* ms) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = wait_reloc(r); if (rc) return rc; }
  if (ms) {
    *ms = -1.0f;
    if (r->timed) ITM_HIP(hipEventElapsedTime(ms, r->ev[0], r->ev[1]));
  }
  if (enable && !r->ev[0]) { ITM_HIP(hipEventCreate(&r->ev[0])); ITM_HIP(hipEventCreate(&r->ev[1])); }
  if (!enable) r->timed = false;
  r->timing = enable != 0;
  return ITM_OK;
}

int itm_reloc_read(itm_reloc* r, float* image_host, uint8_t* code_host) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  if (!r->encoded) return set_error(ITM_ERR_INVALID, "reloc: no code has been encoded yet");
  { const int rc = wait_reloc(r); if (rc) return rc; }
  if (image_host) ITM_HIP(hipMemcpy(image_host, r->image, (size_t)r->ws * r->hs * 4, hipMemcpyDeviceToHost));
  if (code_host) ITM_HIP(hipMemcpy(code_host, r->code, (size_t)r->cfg.numFerns, hipMemcpyDeviceToHost));
  return ITM_OK;
}

int itm_reloc_download(itm_reloc* r, uint8_t* codes_host, float* poses_host) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = wait_reloc(r); if (rc) return rc; }
  if (r->count == 0) return ITM_OK;
  if (codes_host)
    ITM_HIP(hipMemcpy2D(codes_host, (size_t)r->cfg.numFerns, r->db, (size_t)r->rowBytes, (size_t)r->cfg.numFerns, (size_t)r->count, hipMemcpyDeviceToHost));
  if (poses_host) memcpy(poses_host, r->poses.data(), (size_t)r->count * 64);
  return ITM_OK;
}

int itm_reloc_upload(itm_reloc* r, int32_t n, const uint8_t* codes_host, const float* poses_host) {
  if (!r) return set_error(ITM_ERR_INVALID, "null argument");
  if (n < 0 || n > r->cfg.capacity) return set_error(ITM_ERR_INVALID, "reloc: more rows than the database's capacity");
  if (n > 0 && (!codes_host || !poses_host)) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = wait_reloc(r); if (rc) return rc; }
  if (n > 0) {
    std::vector<uint8_t> rows((size_t)n * (size_t)r->rowBytes, 0);      // padded with zeros: the scan counts on it
    for (int i = 0; i < n; ++i) memcpy(rows.data() + (size_t)i * r->rowBytes, codes_host + (size_t)i * r->cfg.numFerns, (size_t)r->cfg.numFerns);
    ITM_HIP(hipMemcpy(r->db, rows.data(), rows.size(), hipMemcpyHostToDevice));
    r->poses.assign(poses_host, poses_host + (size_t)n * 16);
  } else {
    r->poses.clear();
  }
  r->count = n;
  return ITM_OK;
}

int itm_reloc_save(itm_reloc* r, const char* dir) {
  if (!r || !dir) return set_error(ITM_ERR_INVALID, "null argument");
  std::vector<uint8_t> codes((size_t)r->count * (size_t)r->cfg.numFerns);
  { const int rc = itm_reloc_download(r, codes.data(), nullptr); if (rc) return rc; }
  const std::string path = std::string(dir) + kRelocFile, tmp = path + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return set_error(ITM_ERR_INVALID, "reloc: cannot write " + tmp);
  const uint32_t head[2] = {kRelocMagic, 1u};
  const int32_t count = r->count;
  bool ok = fwrite(head, 4, 2, f) == 2 && fwrite(&r->cfg, sizeof r->cfg, 1, f) == 1 && fwrite(&count, 4, 1, f) == 1;
  ok = ok && fwrite(r->pixelHost.data(), 4, r->pixelHost.size(), f) == r->pixelHost.size();
  ok = ok && fwrite(r->thresholdHost.data(), 4, r->thresholdHost.size(), f) == r->thresholdHost.size();
  ok = ok && fwrite(codes.data(), 1, codes.size(), f) == codes.size();
  ok = ok && fwrite(r->poses.data(), 4, (size_t)count * 16, f) == (size_t)count * 16;
  ok = (fclose(f) == 0) && ok;
  if (!ok || rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); return set_error(ITM_ERR_INVALID, "reloc: writing " + path + " failed"); }
  return ITM_OK;
}

int itm_reloc_load(itm_reloc* r, const char* dir) {
  if (!r || !dir) return set_error(ITM_ERR_INVALID, "null argument");
  const std::string path = std::string(dir) + kRelocFile;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return set_error(ITM_ERR_INVALID, "reloc: cannot read " + path);
  auto fail = [&](const char* why) { fclose(f); return set_error(ITM_ERR_INVALID, "reloc: " + path + ": " + why); };
  uint32_t head[2];
  itm_reloc_config cfg;
  int32_t count = 0;
  if (fread(head, 4, 2, f) != 2 || head[0] != kRelocMagic || head[1] != 1u) return fail("not a relocaliser file");
  if (fread(&cfg, sizeof cfg, 1, f) != 1 || fread(&count, 4, 1, f) != 1) return fail("truncated");
  itm_reloc_config mine = r->cfg;
  mine.capacity = cfg.capacity;      // the capacity is the handle's own; everything that shapes a code must agree
  if (memcmp(&mine, &cfg, sizeof cfg) != 0) return fail("written with another configuration");
  if (count < 0 || count > r->cfg.capacity) return fail("more rows than the database's capacity");
  const size_t n = r->pixelHost.size();
  std::vector<int32_t> pixel(n);
  std::vector<float> threshold(n);
  if (fread(pixel.data(), 4, n, f) != n || fread(threshold.data(), 4, n, f) != n) return fail("truncated");
  if (memcmp(pixel.data(), r->pixelHost.data(), n * 4) != 0 || memcmp(threshold.data(), r->thresholdHost.data(), n * 4) != 0) return fail("written with other ferns");
  std::vector<uint8_t> codes((size_t)count * (size_t)r->cfg.numFerns);
  std::vector<float> poses((size_t)count * 16);
  if (fread(codes.data(), 1, codes.size(), f) != codes.size() || fread(poses.data(), 4, poses.size(), f) != poses.size()) return fail("truncated");
  fclose(f);
  return itm_reloc_upload(r, count, codes.data(), poses.data());
}

}  // extern "C"
