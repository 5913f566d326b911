// Host side of the tuning builds' glz_debug_* readers (GLZ_SECTION_TIMES, GLZ_WAVE_TIMES, GLZ_PATH_TIMES; kernels_render.hip,
// kernels_path.hip): the first `bytes` of a __device__ symbol to the host, and the whole symbol zeroed afterwards if asked.
#pragma once
#include <hip/hip_runtime.h>

namespace glz {
template <class Symbol>
static inline int read_device_symbol(void* out, const Symbol& symbol, size_t bytes, int reset) {
  int e = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(symbol), bytes);
  if (reset) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(symbol)) == hipSuccess) e = (int)hipMemset(p, 0, sizeof(Symbol));
  }
  return e;
}
}  // namespace glz
