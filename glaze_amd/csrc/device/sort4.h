// Four 32-bit sort keys in order, in seven instructions: the child sort of a 4-wide node visit (trace_wave, trace_wave_tl).
// The same function compiles for the host, where tests/test_sort4_host.py holds it against std::sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glz {

// minimum, median and maximum of three: on the device one VALU instruction each (v_min3_u32 / v_med3_u32 / v_max3_u32).  clang has no
// builtin for the integer forms (only __builtin_amdgcn_fmed3f), and from min / max written out it selects v_med3_u32 for the median
// but, having found the subexpressions the three share, builds the other two from v_min_u32 / v_max_u32 pairs: ten instructions for the
// sort again.  So the device side names the instructions; they are plain register-to-register VALU operations (no memory, no hazard
// with their neighbours), and the statements are not volatile: the compiler schedules and removes them like any other.
__host__ __device__ inline uint32_t min3_u32(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  const uint32_t m = a < b ? a : b;
  return m < c ? m : c;
#endif
}
__host__ __device__ inline uint32_t max3_u32(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  const uint32_t m = a < b ? b : a;
  return m < c ? c : m;
#endif
}
__host__ __device__ inline uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;   // max(min(a, b), min(max(a, b), c))
  const uint32_t m = hi < c ? hi : c;
  return lo < m ? m : lo;
#endif
}

// a, b, c, d -> ascending (DESCENDING: descending; a pass of any-hit rays, box_key<kKeysFarFirst>).  Three of the keys are put in
// order (lo <= md <= hi), then the fourth finds its place among them: the smallest of all is min(lo, d), the largest max(hi, d), and the
// two in between are the medians of d with the lower and with the upper pair.  The result is the sorted sequence of the four VALUES,
// whatever their multiplicities -- equal keys (several miss markers; hit children never tie, their child bits differ) come out as
// any sorting network leaves them, next to each other.
template <bool DESCENDING = false>
__host__ __device__ inline void sort4(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  const uint32_t lo = min3_u32(a, b, c), md = med3_u32(a, b, c), hi = max3_u32(a, b, c);
  const uint32_t k0 = lo < d ? lo : d, k3 = hi < d ? d : hi;
  const uint32_t k1 = med3_u32(lo, md, d), k2 = med3_u32(md, hi, d);
  a = DESCENDING ? k3 : k0;
  b = DESCENDING ? k2 : k1;
  c = DESCENDING ? k1 : k2;
  d = DESCENDING ? k0 : k3;
}

}  // namespace glz
