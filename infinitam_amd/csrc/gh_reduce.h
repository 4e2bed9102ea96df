// gh_reduce.h -- the deterministic reduction shared by the trackers (tracker.hip: ICP, colour_tracker.hip: photometric,
// ren_tracker.hip: Ren SDF), device and host halves.
//
// One lane per residual accumulates f, the gradient and the packed lower-triangular Hessian in double; a workgroup adds its
// lanes with DPP row shifts and its waves in order and sends one tagged record; the host (or a gathering workgroup) adds the
// records in segments of kSegBlocks workgroups, then the segments in order.  Every path adds in the same order: same bits.
#pragma once

#include <chrono>
#include <cstring>
#include <mutex>

#include "itm_internal.h"
#include "wave_utils.h"

namespace itm {

constexpr int kGHValues = 1 + 6 + 21;   // f, nabla, packed lower-triangular hessian

// Everything the tracker hands between host and device (and between workgroups) travels as TAGGED GRANULES: 8 aligned bytes = 4 bytes
// of payload + the 4-byte sequence number of the evaluation they belong to.  An aligned 8-byte store is indivisible for the device,
// across PCIe and for the host, so a reader that finds the expected number in a granule holds that granule's payload: no stamp
// written after the values, and therefore no wait for the values to have left before the stamp may follow (one PCIe or memory
// round trip per hand-off, 1.5-2 us each, measured).
constexpr int kRecordWords = 2 * kGHValues + 1;   // 28 doubles as two words each, then the count
struct GHBlockRecord { unsigned long long g[64]; };   // one per workgroup (pinned host memory) and the session's result; granule i = tag << 32 | word i
static_assert(kRecordWords <= 64, "record granules");
__host__ __device__ inline unsigned int next_seq(unsigned int s) { ++s; return (s == 0u || s == 0xffffffffu) ? 1u : s; }   // 0 and ~0 are never sequence numbers

// ORDER OF THE ADDITIONS over the workgroups' records, the same wherever they are added (host: per-launch path and coarse levels
// of a session; device: the gathering workgroup of a session), so that every path yields the same bits: records in segments of
// kSegBlocks consecutive workgroups, each segment added up in block order, then the kSegs segment sums in segment order (an
// empty segment contributes +0.0).  A single chain over 240 records was 2.5 us of dependent additions in the gathering workgroup.
constexpr int kSegBlocks = 32;

// thread i < kGHValues holds value i of the workgroup (`mine`); every thread holds `cnt`.  Lane i of the first wave stores granule i:
// one store instruction over 512 contiguous bytes, which leaves the CU as whole 64-byte lines (granules written two per lane,
// 16 bytes apart, crossed PCIe one by one and cost the host's memory a partial-line update each: 7 us per record, measured)
template <int SCOPE>
__device__ inline void send_record(GHBlockRecord* r, double mine, int cnt, unsigned int tag) {
  if (threadIdx.x >= 64) return;
  const int i = threadIdx.x;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(__shfl(mine, i >> 1, 64));
  unsigned int w = (i & 1) ? (unsigned int)(bits >> 32) : (unsigned int)bits;
  if (i == 2 * kGHValues) w = (unsigned int)cnt;
  if (i > 2 * kGHValues) w = 0u;
  __hip_atomic_store(&r->g[i], ((unsigned long long)tag << 32) | w, __ATOMIC_RELAXED, SCOPE);
}

constexpr int kGHGroups = 256;
constexpr int kSegs = (kGHGroups + kSegBlocks - 1) / kSegBlocks;
constexpr int kGHWaves = 4;      // waves per workgroup (measured per 640x480 evaluation: 4 waves 43 us, 8 waves 51 us, 16 waves 73 us)
static_assert(kSegBlocks % kGHWaves == 0, "a gathering workgroup splits its segment evenly over its waves");
constexpr int kGHThreads = 64 * kGHWaves;

// Sum of `s` over the 64 lanes of the wave, the same value in every lane: an inclusive scan inside each row of 16 lanes with DPP
// row shifts (lanes that would read from outside their row add 0), then the four row totals in row order.  Data-parallel
// primitives keep the exchange in the ALU; the ds_bpermute butterfly this replaces was one LDS round trip per step and value
// (2.7 us per evaluation for the block reduction, measured).  The order of the additions is fixed: deterministic sums.
template <int CTRL>
__device__ inline double dpp_shifted(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)b, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned int)(b >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo));
}
__device__ inline double lane_value(double v, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)b, lane), hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ inline double wave_sum(double s) {
  s += dpp_shifted<0x111>(s);   // row_shr:1
  s += dpp_shifted<0x112>(s);   // row_shr:2
  s += dpp_shifted<0x114>(s);   // row_shr:4
  s += dpp_shifted<0x118>(s);   // row_shr:8  -> lane 15 of every row holds the row's sum
  return ((lane_value(s, 15) + lane_value(s, 31)) + lane_value(s, 47)) + lane_value(s, 63);
}

// wave sums in double (fixed order), then the waves in order: thread i < kGHValues ends up with value i of the workgroup, every
// thread with its count
template <int MODE>
__device__ inline void gh_block_reduce(const double acc[kGHValues], int valid, double (*lds)[kGHValues], int* ldsCount, double& mine, int& cnt) {
  constexpr int NP = (MODE == 3) ? 6 : 3;
  constexpr int NH = NP * (NP + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kGHValues; ++i) {
    const bool used = (i == 0) || (i >= 1 && i < 1 + NP) || (i >= 7 && i < 7 + NH);
    const double s = used ? wave_sum(acc[i]) : 0.0;
    if (lane == 0) lds[wave][i] = s;
  }
  const int total = wave_reduce_sum(valid);
  if (lane == 0) ldsCount[wave] = total;
  __syncthreads();
  mine = 0.0; cnt = 0;
#pragma unroll
  for (int wv = 0; wv < kGHWaves; ++wv) {          // fixed order: deterministic
    if (threadIdx.x < kGHValues) mine += lds[wv][threadIdx.x];
    cnt += ldsCount[wv];
  }
}

// the common order of the additions (kSegBlocks above) on the host
struct OrderedSums {
  double seg[kSegs][kGHValues];
  OrderedSums() { for (int g = 0; g < kSegs; ++g) for (int i = 0; i < kGHValues; ++i) seg[g][i] = 0.0; }
  double* of_block(size_t b) { return seg[b / kSegBlocks]; }
  void total(double out[kGHValues]) const {
    for (int i = 0; i < kGHValues; ++i) {
      double s = 0.0;
      for (int g = 0; g < kSegs; ++g) s += seg[g][i];
      out[i] = s;
    }
  }
};

// Adds one tagged record to `sums` / `count` once every granule carries `tag`.  `slow(granule)` is called every 1024 polls of a
// granule that has not arrived and decides whether the wait goes on (ITM_OK) or ends with an error code.
template <class Slow>
static inline int read_record(const GHBlockRecord* r, unsigned int tag, double* sums, int* count, Slow&& slow) {
  unsigned int w[kRecordWords];
  for (int i = 0; i < kRecordWords; ++i) {
    const volatile unsigned long long* g = &r->g[i];
    unsigned long long v;
    unsigned spins = 0;
    while ((unsigned int)((v = *g) >> 32) != tag) {
      __builtin_ia32_pause();
      if ((++spins & 0x3ffu) != 0u) continue;
      const int rc = slow(g);
      if (rc) return rc;
    }
    w[i] = (unsigned int)v;
  }
  for (int i = 0; i < kGHValues; ++i) {
    const unsigned long long bits = (unsigned long long)w[2 * i] | ((unsigned long long)w[2 * i + 1] << 32);
    double d;
    memcpy(&d, &bits, 8);
    sums[i] += d;
  }
  *count += (int)w[2 * kGHValues];
  return ITM_OK;
}

// Waits for the records of `blocks` workgroups tagged `seq` (pinned host memory) and adds them in the common order.  The poll is
// bounded in TIME: after 20 ms without a granule the stream is queried between polls -- a drained stream without it, a device
// error, or kPollTimeoutSeconds without progress end the call with ITM_ERR_DEVICE instead of stalling the host on a kernel that
// will never finish.
constexpr double kPollTimeoutSeconds = 5.0;
static inline int collect_records(const GHBlockRecord* rec, size_t blocks, unsigned int seq, hipStream_t st, double sums[kGHValues], int* n) {
  OrderedSums ordered;
  *n = 0;
  using clock = std::chrono::steady_clock;
  clock::time_point t0; bool timing = false;
  for (size_t b = 0; b < blocks; ++b) {
    const int rc = read_record(rec + b, seq, ordered.of_block(b), n, [&](const volatile unsigned long long* g) -> int {
      if (!timing) { t0 = clock::now(); timing = true; return ITM_OK; }
      const double waited = std::chrono::duration<double>(clock::now() - t0).count();
      if (waited < 0.02) return ITM_OK;
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) {
        if ((unsigned int)(*g >> 32) == seq) return ITM_OK;
        return set_error(ITM_ERR_DEVICE, "tracker reduction: the stream drained without delivering every record");
      }
      if (q != hipErrorNotReady) return hip_fail(q, "tracker reduction", __FILE__, __LINE__);
      if (waited > kPollTimeoutSeconds) return set_error(ITM_ERR_DEVICE, "tracker reduction timed out");
      return ITM_OK;
    });
    if (rc) return rc;
  }
  ordered.total(sums);
  return ITM_OK;
}

// A tracker handle's end of the reduction: the pinned records its launches send (coherent + mapped: device stores become visible
// to the polling host without a kernel boundary), the device they live on and the handle's sequence numbers.  One channel per
// handle, so two handles never share records or sequence numbers.
struct GHChannel {
  PinnedBuffer<GHBlockRecord> rec;   // pinned host records (capacity in workgroups) and their device address
  int device = -1;                   // the device of the last reserve
  unsigned int seq = 0;
  unsigned int round = 0;            // times the numbers have started over (what a holder of further tagged records compares: tracker.hip)

  // the current device is not the one the records were reserved on: the handle's other buffers are of no use here either
  bool moved() const { int dev = 0; (void)hipGetDevice(&dev); return dev != device; }
  void release() { rec.reset(); }
  // at least `blocks` records on the current device (grows only); on failure the channel holds none
  int reserve(size_t blocks) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev == device && rec.capacity() >= blocks) return ITM_OK;
    device = dev;
    const hipError_t e = rec.alloc(blocks, hipHostMallocMapped | hipHostMallocCoherent, true);
    if (e != hipSuccess) return hip_fail(e, "tracker records", __FILE__, __LINE__);
    return ITM_OK;
  }
  bool wraps() const { return next_seq(seq) < seq; }      // the next evaluation starts the numbers over
  // The tag of the next evaluation's records.  When the numbers start over the records are cleared (tag 0: no record): the record of a
  // workgroup that only large evaluations reach keeps the tag of the last one, and the new round hands that number out again.  Nothing
  // is in flight here: every evaluation before this one has been collected, i.e. every record it sent has arrived.
  unsigned int begin() {
    if (wraps()) {
      if (rec) memset((void*)rec.get(), 0, rec.capacity() * sizeof(GHBlockRecord));
      ++round;
    }
    return seq = next_seq(seq);
  }
  int collect(size_t blocks, unsigned int tag, hipStream_t st, double sums[kGHValues], int* n) const {
    return collect_records(rec, blocks, tag, st, sums, n);
  }
};

// What every handle that owns a channel begins with: the mutex that serialises its callers, the channel, and the host frame of an
// evaluation that is ONE launch.  The order of the steps is the contract of the tagged records: the tag is taken before the launch
// that sends it, and the host waits for exactly as many records as workgroups were launched.
struct GHHandle {
  mutable std::mutex mu;
  GHChannel ch;

  // Records for `blocks` workgroups on the current device; `release` (the handle's own: the channel and whatever else it holds on a
  // device) runs first when the handle's memory is that of another device.
  template <class Release>
  int ready(Release&& release, size_t blocks = kGHGroups) {
    if (ch.moved()) release();
    return ch.reserve(blocks);
  }
  // launch(records, tag) starts `groups` workgroups on st, each of which sends one record with that tag, and returns ITM_OK or an
  // error of its own; sums / *valid receive the records' values and counts, added in the common order.
  template <class Launch>
  int evaluate(size_t groups, hipStream_t st, Launch&& launch, double sums[kGHValues], int* valid) {
    const unsigned int seq = ch.begin();
    { const int rc = launch(ch.rec.device(), seq); if (rc) return rc; }
    ITM_LAUNCH_CHECK();
    return ch.collect(groups, seq, st, sums, valid);
  }
  // itm_debug_counter's view of ch.seq: *get receives it, then *set replaces it
  int seq_counter(const uint32_t* set, uint32_t* get) {
    std::lock_guard<std::mutex> lock(mu);
    if (get) *get = ch.seq;
    if (set) ch.seq = *set;
    return ITM_OK;
  }
};
// the handle types as their base, each converted where the type is complete (the compiler checks the conversion); null stays null
GHHandle* gh_handle(itm_colour_tracker* t);            // colour_tracker.hip
GHHandle* gh_handle(itm_ren_tracker* t);               // ren_tracker.hip
GHHandle* gh_handle(itm_pose_quality_handle* q);       // pose_quality.hip
GHHandle* gh_handle(itm_aligner* a);                   // align.hip

// The gradient nabla[0..np) and the symmetric Hessian hessian[r + c * ld] (column-major) from the sums, each times `scale`.
// Scale 1 stores the bits of the plain (float) conversion: multiplying by 1.0f is exact.
static inline void unpack_gh(const double sums[kGHValues], int np, int ld, float scale, float* nabla, float* hessian) {
  for (int r = 0, k = 0; r < np; ++r) {
    nabla[r] = (float)sums[1 + r] * scale;
    for (int c = 0; c <= r; ++c, ++k) hessian[r + c * ld] = (float)sums[7 + k] * scale;
  }
  for (int r = 0; r < np; ++r)
    for (int c = r + 1; c < np; ++c) hessian[r + c * ld] = hessian[c + r * ld];
}

}  // namespace itm
