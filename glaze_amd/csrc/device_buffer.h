// The one owner of device memory in csrc: a typed hipMalloc'ed array, freed when it goes out of scope.  Movable, not copyable.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace glz {

template <class T>
struct DeviceBuffer {
  T* ptr = nullptr;
  size_t count = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), count(o.count) {
    o.ptr = nullptr;
    o.count = 0;
  }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      release();
      ptr = o.ptr;
      count = o.count;
      o.ptr = nullptr;
      o.count = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  void release() {   // hipFree waits for the device: work in flight on the buffer has ended when it returns
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    count = 0;
  }
  hipError_t alloc(size_t n) {
    release();
    count = n;
    return hipMalloc(reinterpret_cast<void**>(&ptr), sizeof(T) * (n ? n : 1));
  }
  hipError_t upload(const T* host, size_t n, hipStream_t st) {
    hipError_t e = alloc(n);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(ptr, host, sizeof(T) * n, hipMemcpyHostToDevice, st);
  }
};

// buffers of n entries each; the first error ends it
template <class... Buffers>
inline hipError_t alloc_each(size_t n, Buffers&... buffers) {
  hipError_t e = hipSuccess;
  ((e = e == hipSuccess ? buffers.alloc(n) : e), ...);
  return e;
}

}  // namespace glz
