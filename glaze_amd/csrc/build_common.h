// What the scene-build translation units (kernels_build.hip, kernels_build_sah.hip, kernels_records.hip) share.  Internal: only they include it.
#pragma once
#include <hip/hip_runtime.h>

#define GLZ_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

namespace glz {

// launches a kernel and reports what the launch said (conversions to the kernel's parameter types happen at the launch)
template <class Kernel, class... Args>
inline hipError_t launch(Kernel kernel, dim3 grid, dim3 block, hipStream_t st, Args... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
  return hipGetLastError();
}

// floats as ints that compare like the floats: min / max of coordinates with integer atomics
__device__ __forceinline__ int float_to_ordered(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float ordered_to_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

__host__ __device__ __forceinline__ float box_area(float4 l, float4 h) {
  const float dx = h.x - l.x, dy = h.y - l.y, dz = h.z - l.z;
  return 2.0f * (dx * dy + dy * dz + dz * dx);
}
// centre of a box: whole, and on one axis
__device__ __forceinline__ void box_centroid(float4 l, float4 h, float* c) {
  c[0] = 0.5f * (l.x + h.x); c[1] = 0.5f * (l.y + h.y); c[2] = 0.5f * (l.z + h.z);
}
__device__ __forceinline__ float box_centroid(float4 l, float4 h, int axis) {
  return axis == 0 ? 0.5f * (l.x + h.x) : (axis == 1 ? 0.5f * (l.y + h.y) : 0.5f * (l.z + h.z));
}

// The binned SAH builder on the device (kernels_build_sah.hip): fills children / parent (links >= 0 inner node, < 0 ~leaf; parent by
// box slot, leaf j at (n-1)+j) over the n >= 2 leaf boxes leaf_lo / leaf_hi, one or seven launches and one synchronisation per level.
hipError_t build_sah_levels(hipStream_t st, uint32_t n, const float4* leaf_lo, const float4* leaf_hi, int2* children, int* parent);

}  // namespace glz
