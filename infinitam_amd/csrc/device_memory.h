// device_memory.h -- the two owners of everything the library allocates: DeviceBuffer<T> (hipMalloc) and PinnedBuffer<T>
// (hipHostMalloc, with the device address of mapped memory).  Host code only.  Both are move-only, free in their destructors and go
// through the one pair memory_alloc / memory_free below; no other file of the library calls the runtime's allocation functions
// (the four raw entry points of scene.hip, which hand memory to the host, excepted).  Nothing is pooled or cached: a buffer is
// allocated and freed exactly where its owner says.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>

namespace itm {

// What passed through the pair, process-wide (itm_debug_memory), and ITM_DEBUG_FAIL_ALLOCATION's countdown.
struct MemoryStats {
  std::atomic<int64_t> live{0}, liveBytes{0}, attempted{0};
  std::atomic<int64_t> failAt{0};      // n > 0: the n-th attempt from now fails (once); 0: off
};
inline MemoryStats& memory_stats() { static MemoryStats m; return m; }

// pinned: hipHostMalloc with `flags`; otherwise hipMalloc, or hipExtMallocWithFlags when `flags` asks for a kind of device memory.
// *p is null on failure.
inline hipError_t memory_alloc(void** p, size_t bytes, bool pinned, unsigned flags = 0) {
  MemoryStats& m = memory_stats();
  *p = nullptr;
  m.attempted.fetch_add(1);
  if (m.failAt.load() > 0 && m.failAt.fetch_sub(1) == 1) return hipErrorOutOfMemory;      // (the runtime is not called: nothing sticky)
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, flags) : flags ? hipExtMallocWithFlags(p, bytes, flags) : hipMalloc(p, bytes);
  if (e != hipSuccess) { *p = nullptr; return e; }
  m.live.fetch_add(1); m.liveBytes.fetch_add((int64_t)bytes);
  return hipSuccess;
}
inline void memory_free(void* p, size_t bytes, bool pinned) {
  if (!p) return;
  (void)(pinned ? hipHostFree(p) : hipFree(p));
  MemoryStats& m = memory_stats();
  m.live.fetch_sub(1); m.liveBytes.fetch_sub((int64_t)bytes);
}

template <class T> struct ElementBytes { static constexpr size_t value = sizeof(T); };
template <> struct ElementBytes<void> { static constexpr size_t value = 1; };

// The state and the moves the two owners share; PINNED selects the half of the pair.
template <class T, bool PINNED>
class OwnedMemory {
 public:
  OwnedMemory() = default;
  OwnedMemory(const OwnedMemory&) = delete;
  OwnedMemory& operator=(const OwnedMemory&) = delete;
  OwnedMemory(OwnedMemory&& o) noexcept : p_(o.p_), dev_(o.dev_), n_(o.n_), bytes_(o.bytes_) { o.p_ = nullptr; o.dev_ = nullptr; o.n_ = 0; o.bytes_ = 0; }
  OwnedMemory& operator=(OwnedMemory&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; dev_ = o.dev_; n_ = o.n_; bytes_ = o.bytes_; o.p_ = nullptr; o.dev_ = nullptr; o.n_ = 0; o.bytes_ = 0; }
    return *this;
  }
  ~OwnedMemory() { reset(); }

  void reset() { memory_free((void*)p_, bytes_, PINNED); p_ = nullptr; dev_ = nullptr; n_ = 0; bytes_ = 0; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t capacity() const { return n_; }      // in elements
  size_t bytes() const { return bytes_; }     // as allocated (an empty request is rounded up)

 protected:
  hipError_t allocate(size_t n, size_t emptyBytes, unsigned flags) {
    reset();
    const size_t want = n * ElementBytes<T>::value;
    void* q = nullptr;
    const hipError_t e = memory_alloc(&q, want ? want : emptyBytes, PINNED, flags);
    if (e == hipSuccess) { p_ = (T*)q; n_ = n; bytes_ = want ? want : emptyBytes; }
    return e;
  }
  T* p_ = nullptr;
  T* dev_ = nullptr;      // PinnedBuffer: the device address of mapped memory
  size_t n_ = 0, bytes_ = 0;
};

// Device memory.  Converts to T* so that launch lines and memsets read as they do with a raw pointer.
template <class T>
class DeviceBuffer : public OwnedMemory<T, false> {
 public:
  // exactly n elements, whatever was held before is freed first; an empty request still allocates `emptyBytes`;
  // `flags`: those of hipExtMallocWithFlags (fine-grained memory), 0 for plain device memory
  hipError_t alloc(size_t n, size_t emptyBytes = 16, unsigned flags = 0) { return this->allocate(n, emptyBytes, flags); }
  // at least n elements: grows only, contents are not kept; on failure the buffer is empty
  hipError_t reserve(size_t n) { return (this->p_ && n <= this->n_) ? hipSuccess : alloc(n); }
};

// Page-locked host memory.  With hipHostMallocMapped in `flags` it also holds the address the device uses, and an allocation
// whose device address cannot be had fails as a whole.
template <class T>
class PinnedBuffer : public OwnedMemory<T, true> {
 public:
  hipError_t alloc(size_t n, unsigned flags, bool zeroFill = false, size_t emptyBytes = 1) {
    hipError_t e = this->allocate(n, emptyBytes, flags);
    if (e != hipSuccess) return e;
    if (zeroFill) memset((void*)this->p_, 0, this->bytes_);
    if (flags & hipHostMallocMapped) {
      void* d = nullptr;
      e = hipHostGetDevicePointer(&d, (void*)this->p_, 0);
      if (e != hipSuccess) { this->reset(); return e; }
      this->dev_ = (T*)d;
    }
    return hipSuccess;
  }
  T* device() const { return this->dev_; }
};

}  // namespace itm
