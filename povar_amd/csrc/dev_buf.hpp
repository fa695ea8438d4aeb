// dev_buf.hpp -- DevBuf<T>: a device allocation that frees itself.  Not copyable; a move leaves the source empty, so std::swap
// of two buffers (and of two structs of buffers) exchanges them without a free.  p and n are public: the call sites read them.
#pragma once
#include <hip/hip_runtime_api.h>

#include <type_traits>
#include <utility>

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      n = std::exchange(o.n, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  // `count` elements in place of whatever the buffer owns (0: nothing).  *total grows by the new bytes on success; taking the old
  // ones off is the caller's business.  On a failure the buffer is empty.
  hipError_t alloc(size_t count, size_t* total) {
    release();
    if (count == 0) return hipSuccess;
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count;
    if (total) *total += count * sizeof(T);
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf<int>> && !std::is_copy_assignable_v<DevBuf<int>>);
