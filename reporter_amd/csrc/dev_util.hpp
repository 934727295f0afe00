// dev_util.hpp — the host-side HIP plumbing the engine, the matcher, the C API and the stages
// around them share: device and pinned buffers that free themselves, HIP-event part timers, the
// hipcub scan / sort scratch, grid() and
// the iota / fill kernels.  Growth policy stays with the callers: a buffer is given the capacity
// its owner computed.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "serve_policy.hpp"

namespace rm {

#define RM_HIP(x)                                                                                \
  do {                                                                                           \
    hipError_t _e = (x);                                                                         \
    if (_e != hipSuccess)                                                                        \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #x);   \
  } while (0)

// hipMalloc found too little free HBM (the engine's allocator; callers decide whether a smaller
// request can succeed: workspaces turn it into BatchTooLarge, the route-ball build steps down)
struct OutOfDeviceMemory : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// blocks of b threads over n items, at least one (every kernel launched through it checks its index)
inline uint32_t grid(uint64_t n, uint32_t b = 256) { return (uint32_t)std::max<uint64_t>((n + b - 1) / b, 1); }

template <class I>
__global__ void k_iota(I n, uint32_t* v) {
  const I k = (I)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) v[k] = (uint32_t)k;
}
template <class T>
__global__ void k_fill(uint32_t n, T* v, T x) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) v[k] = x;
}

// A typed device allocation that frees itself; converts to its pointer.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(uint64_t cap) { reserve(cap); }
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~DevBuf() { reset(); }
  // A new block of `cap` elements (at least one).  keep == kDiscard: the old block goes first,
  // with its contents (an owner that tracks a capacity of its own zeroes it before the call).
  // Any other keep: the new block is taken first, the old one's first `keep` elements move by a
  // device copy on st, and st is synchronised before the old block is freed.  A full HBM clears
  // the error and throws BatchTooLarge(too_large), or OutOfDeviceMemory where the caller names no
  // message; a keeping call has then changed nothing.
  static constexpr uint64_t kDiscard = ~0ull;
  void reserve(uint64_t cap, const char* too_large = nullptr, uint64_t keep = kDiscard, hipStream_t st = nullptr) {
    if (keep == kDiscard) reset();
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<uint64_t>(cap, 1) * sizeof(T));
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      if (too_large) throw BatchTooLarge(too_large);
      throw OutOfDeviceMemory("out of device memory allocating " + std::to_string(std::max<uint64_t>(cap, 1) * sizeof(T)) + " bytes");
    }
    RM_HIP(e);
    if (p_) {   // (a keeping call)
      hipError_t c = keep ? hipMemcpyAsync(q, p_, keep * sizeof(T), hipMemcpyDeviceToDevice, st) : hipSuccess;
      if (c == hipSuccess) c = hipStreamSynchronize(st);
      if (c != hipSuccess) (void)hipFree(q);
      RM_HIP(c);
      reset();
    }
    p_ = (T*)q;
    cap_ = cap;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  uint64_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  uint64_t cap_ = 0;
};

// The same in pinned host memory (contents are never kept: the old block always goes first).
template <class T>
class PinBuf {
 public:
  PinBuf() = default;
  PinBuf(PinBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  PinBuf& operator=(PinBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
  ~PinBuf() { reset(); }
  // memory that cannot be pinned throws BatchTooLarge(too_large) where the caller names a message
  void reserve(uint64_t cap, const char* too_large = nullptr) {
    const hipError_t e = try_reserve(cap);
    if (e == hipErrorOutOfMemory && too_large) throw BatchTooLarge(too_large);
    RM_HIP(e);
  }
  // the same for a caller with a second size to try: a failure is returned with the error cleared
  // and the buffer empty
  hipError_t try_reserve(uint64_t cap) {
    reset();
    const hipError_t e = hipHostMalloc((void**)&p_, std::max<uint64_t>(cap, 1) * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); p_ = nullptr; return e; }
    cap_ = cap;
    return hipSuccess;
  }
  void reset() {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  operator T*() const { return p_; }
  T* get() const { return p_; }
  uint64_t cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  uint64_t cap_ = 0;
};

// HIP-event pairs around the parts of a call, pooled: a part may be timed several times.
class PartTimer {
 public:
  PartTimer() = default;
  PartTimer(const PartTimer&) = delete;
  PartTimer& operator=(const PartTimer&) = delete;
  ~PartTimer() {
    for (Ev& e : pending_) { free_.push_back(e.a); free_.push_back(e.b); }
    for (hipEvent_t e : free_) (void)hipEventDestroy(e);
  }
  void tic(int part, hipStream_t st) {
    Ev e{event(), event(), part};
    pending_.push_back(e);
    RM_HIP(hipEventRecord(e.a, st));
  }
  void toc(hipStream_t st) {
    if (!pending_.empty()) RM_HIP(hipEventRecord(pending_.back().b, st));
  }
  // after a stream synchronise: every pair's time is added to ms[its part] (null: dropped), and
  // pairs[its part] counts it
  void harvest(double* ms, uint64_t* pairs = nullptr) {
    for (Ev& e : pending_) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, e.a, e.b) != hipSuccess) (void)hipGetLastError();   // (a part an exception cut short)
      else if (ms) { ms[e.part] += t; if (pairs) pairs[e.part] += 1; }
      free_.push_back(e.a); free_.push_back(e.b);
    }
    pending_.clear();
  }

 private:
  struct Ev { hipEvent_t a, b; int part; };
  std::vector<Ev> pending_;
  std::vector<hipEvent_t> free_;
  hipEvent_t event() {
    hipEvent_t e;
    if (!free_.empty()) { e = free_.back(); free_.pop_back(); return e; }
    RM_HIP(hipEventCreate(&e));
    return e;
  }
};

// hipcub's scratch: size query, growth, run.  The old scratch may still be in flight on the
// stream, so it is freed only after a stream synchronise.  Every member that names a hipcub
// algorithm is a template, so only the files that scan or sort carry hipcub's kernels.
class ScanScratch {
 public:
  explicit ScanScratch(const char* too_large = nullptr) : too_large_(too_large) {}
  template <class T>
  void scan(const T* in, T* out, uint64_t n, hipStream_t st) {
    run([&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, (int)n, st); }, st);
  }
  template <class K>
  void sort_pairs(const K* kin, K* kout, const uint32_t* vin, uint32_t* vout, uint64_t n, int bits, hipStream_t st) {
    run([&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, kin, kout, vin, vout, (int)n, 0, bits, st); }, st);
  }
  template <class K>
  void sort_keys(const K* in, K* out, uint64_t n, hipStream_t st) {
    run([&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortKeys(t, b, in, out, (int)n, 0, 64, st); }, st);
  }
  // room for the 32-bit scans (and with kSorts the pair sorts) of up to n items, taken ahead: a
  // full HBM shows before the call writes anything, and no scan or sort of the call grows the
  // scratch (and synchronises) between its kernels
  template <bool kSorts, class K = unsigned long long>
  void presize(uint64_t n, hipStream_t st) {
    size_t a = 0, b = 0;
    if constexpr (kSorts)
      RM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, a, (K*)nullptr, (K*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                (int)n, 0, 64, st));
    RM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, st));
    need(std::max(a, b), st);
  }

 private:
  DevBuf<char> tmp_;
  const char* too_large_;
  void need(size_t b, hipStream_t st) {
    if (b <= tmp_.cap() && tmp_) return;
    if (tmp_) RM_HIP(hipStreamSynchronize(st));
    tmp_.reserve(b + b / 2 + 256, too_large_);
  }
  template <class F>
  void run(F f, hipStream_t st) {
    size_t b = 0;
    RM_HIP(f(nullptr, b));
    need(b, st);
    b = tmp_.cap();
    RM_HIP(f(tmp_.get(), b));
  }
};

}  // namespace rm
