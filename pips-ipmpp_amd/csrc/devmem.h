// Owners of device and pinned host memory.  Every allocation of the library is held by one of these two types: it is declared
// once, freed by its owner's destructor and counted while it lives (pips_hip_device_allocs_live / _bytes_live), so that "nothing
// leaks" is a number a test can assert.  No pool, no cache: one alloc() is one hipMalloc, one reset() one hipFree (which
// synchronises the device, as it always did).  Only in translation units that include the HIP runtime (after common.h).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <vector>

#include "common.h"

namespace pips {

inline std::atomic<long long> g_mem_allocs_live{0}, g_mem_bytes_live{0};   // device and pinned together

template <class T, bool Pinned>
class MemBuf {
   T* p_ = nullptr;
   size_t n_ = 0;   // elements allocated (at least one while p_ is set)

public:
   MemBuf() = default;
   MemBuf(const MemBuf&) = delete;
   MemBuf& operator=(const MemBuf&) = delete;
   MemBuf(MemBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
   MemBuf& operator=(MemBuf&& o) noexcept {
      if (this != &o) {
         reset();
         p_ = o.p_; n_ = o.n_;
         o.p_ = nullptr; o.n_ = 0;
      }
      return *this;
   }
   ~MemBuf() { reset(); }

   void reset() {
      if (!p_) return;
      (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
      g_mem_allocs_live.fetch_sub(1, std::memory_order_relaxed);
      g_mem_bytes_live.fetch_sub((long long)(n_ * sizeof(T)), std::memory_order_relaxed);
      p_ = nullptr; n_ = 0;
   }
   // max(n, 1) elements (an empty array still has a non-null pointer); what was held before is freed first
   int alloc(size_t n) {
      reset();
      n = std::max<size_t>(n, 1);
      void* q = nullptr;
      const hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
      if (e != hipSuccess)
         PIPS_FAIL(PIPS_ERR_HIP, "%s(%zu bytes) failed: %s (%s:%d)", Pinned ? "hipHostMalloc" : "hipMalloc", n * sizeof(T), hipGetErrorString(e), __FILE__, __LINE__);
      p_ = (T*)q; n_ = n;
      g_mem_allocs_live.fetch_add(1, std::memory_order_relaxed);
      g_mem_bytes_live.fetch_add((long long)(n * sizeof(T)), std::memory_order_relaxed);
      return PIPS_OK;
   }
   int alloc_zero(size_t n) {
      if (int rc = alloc(n)) return rc;
      const hipError_t e = hipMemset(p_, 0, n_ * sizeof(T));
      if (e != hipSuccess) PIPS_FAIL(PIPS_ERR_HIP, "hipMemset failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      return PIPS_OK;
   }
   // a fresh allocation holding h (a blocking, counted copy)
   int upload(const std::vector<T>& h) {
      if (int rc = alloc(h.size())) return rc;
      if (h.empty()) return PIPS_OK;
      const hipError_t e = hipMemcpy(p_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
      if (e != hipSuccess) PIPS_FAIL(PIPS_ERR_HIP, "hipMemcpy failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
      return PIPS_OK;
   }
   // buffers kept between calls: grows only (free, then allocate larger); the contents are not carried over
   int reserve(size_t n) { return p_ && n <= n_ ? PIPS_OK : alloc(n); }

   size_t size() const { return n_; }
   T* get() const { return p_; }
   operator T*() const { return p_; }   // launches, pointer arithmetic and null tests read as with a raw pointer
};

template <class T> using DevBuf = MemBuf<T, false>;      // hipMalloc / hipFree
template <class T> using PinnedBuf = MemBuf<T, true>;    // hipHostMalloc(hipHostMallocDefault) / hipHostFree

}  // namespace pips
