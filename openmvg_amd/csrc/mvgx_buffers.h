// Growable buffers that own their memory: DevBuf<T> (device, straight from device_malloc) and PinnedBuf<T> (page-locked host, or
// plain host memory on request). A buffer frees itself when it goes out of scope or its context is deleted, so a context needs no
// release list. Kernels are handed the raw pointer `p` (the test-suite's emulation captures launch arguments by value), hence no copies.
// What sub-allocates from an Arena (DevArray in mvgx_guided.hip, dev_alloc / dev_upload* in mvgx_ba.hip) is a different thing and lives there.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "mvgx_common.h"

namespace mvgx {

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  bool headroom_quarter = false;   // true: a regrow asks for n + n / 4 elements (mvgx_bruteforce.hip, whose batch lists vary in length)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // at least n elements; the old content is NOT kept
  int ensure(size_t n) {
    if (n <= cap) return MVGX_OK;
    release();
    const size_t want = std::max<size_t>(headroom_quarter ? n + n / 4 : n, 16);
    MVGX_HIP(device_malloc(reinterpret_cast<void**>(&p), want * sizeof(T)));
    cap = want;
    return MVGX_OK;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
};

template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  bool headroom_quarter = false;   // as in DevBuf
  bool pageable = false;   // true: plain malloc'd memory (cheap to obtain; D2H copies are staged by the runtime); grow_keep only
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  int ensure(size_t n) {
    if (n <= cap) return MVGX_OK;
    release();
    const size_t want = std::max<size_t>(headroom_quarter ? n + n / 4 : n, 16);
    MVGX_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), want * sizeof(T), hipHostMallocDefault));
    cap = want;
    return MVGX_OK;
  }
  // grow to at least n elements, keeping the first `used` (geometric growth: the caller appends batch after batch)
  int grow_keep(size_t n, size_t used) {
    if (n <= cap) return MVGX_OK;
    const size_t want = std::max<size_t>(std::max<size_t>(n, cap + cap / 2), 16);
    if (pageable) {
      T* q = static_cast<T*>(realloc(p, want * sizeof(T)));
      MVGX_REQUIRE(q != nullptr, MVGX_ERR_HIP, "out of host memory (%zu bytes)", want * sizeof(T));
      p = q;
      cap = want;
      return MVGX_OK;
    }
    T* q = nullptr;
    MVGX_HIP(hipHostMalloc(reinterpret_cast<void**>(&q), want * sizeof(T), hipHostMallocDefault));
    if (p) {
      if (used) memcpy(q, p, used * sizeof(T));
      (void)hipHostFree(p);
    }
    p = q;
    cap = want;
    return MVGX_OK;
  }
  void release() { if (p) { if (pageable) free(p); else (void)hipHostFree(p); p = nullptr; cap = 0; } }
};

}  // namespace mvgx
