// Host side of the kernels' launch geometry: one block per kBlock items, and how many blocks of a persistent kernel the device holds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"

namespace glz {

// one thread per item, kTraceBlock to a block; nothing is launched for n = 0
static inline dim3 grid_for(uint32_t n) { return dim3((n + kTraceBlock - 1) / kTraceBlock); }
template <class Kernel, class... Args>
static inline hipError_t launch_per_item(hipStream_t st, Kernel kernel, uint32_t n, Args... args) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, grid_for(n), dim3(kTraceBlock), 0, st, args...);
  return hipGetLastError();
}

// Blocks of `kernel` (kTraceBlock threads, `dyn_lds` bytes of dynamic LDS) that are resident at once on the current device: CUs x
// blocks per CU from the occupancy query (`fallback` when it fails), at most kPersistentBlocksPerCuMax and at most `cap` per CU.
template <class Kernel>
static inline uint32_t resident_blocks(Kernel kernel, size_t dyn_lds, int fallback, int cap = kPersistentBlocksPerCuMax) {
  int dev = 0, cus = 256, per_cu = 0;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)kTraceBlock, dyn_lds) != hipSuccess || per_cu < 1) per_cu = fallback;
  return (uint32_t)cus * (uint32_t)std::max(1, std::min({per_cu, kPersistentBlocksPerCuMax, cap}));
}

// for every kernel built on trace_wave / trace_wave_tl (kernels_render.hip, kernels_post.hip, kernels_debug.hip)
// Persistent tracers: the grid is exactly what is resident at once (CUs x blocks per CU from the occupancy query, at
// most 8), and never more waves than there are 64-ray groups.  A block that had to wait for a slot would serialise
// behind a whole persistent block (cdna_hip_programming.md section 1: size persistent grids by residency).
template <class Kernel>
static inline dim3 persistent_grid(Kernel kernel, uint32_t n_rays) {
  const char* cap = getenv("GLAZE_TRACE_BLOCKS_PER_CU");   // tuning: leave room for another chain's k_shade
  // (splitting the resident blocks between concurrent chains measured slower: a chain's blocks fill in as another's retire)
  const uint32_t resident = resident_blocks(kernel, 0, 4, cap ? atoi(cap) : 8);
  return dim3(std::max<uint32_t>(1u, std::min<uint32_t>((n_rays + kTraceBlock - 1) / kTraceBlock, resident)));
}

}  // namespace glz
