// Instance boxes of a two-level scene's top level on the device (Scene::update_transforms): the world AABB of each instance's mesh
// vertices in double precision, padded by the rule of host_instance_boxes (scene.cpp), bit for bit.
#include <hip/hip_runtime.h>

#include "device/types.h"
#include "kernels.h"

namespace glz {

namespace {
constexpr uint32_t kBoxBlock = 256;   // four waves, one work item (InstanceBoxItem) / one instance each

// std::min(a, b) / std::max(a, b) of the host rule: the first argument unless the second compares below / above it, so a NaN
// second argument is skipped.  The running values start at +-1e300 and only ever take a non-NaN point, never a NaN.
__device__ __forceinline__ double min_first(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double max_first(double a, double b) { return a < b ? b : a; }

// std::nextafterf(x, -INFINITY) / (x, INFINITY) for x that is not NaN (k_instance_box_finish never has one)
__device__ __forceinline__ float next_down(float x) {
  const uint32_t b = __float_as_uint(x);
  if (x == -INFINITY) return x;
  if (x == 0.0f) return __uint_as_float(0x80000001u);
  return __uint_as_float(x > 0.0f ? b - 1u : b + 1u);
}
__device__ __forceinline__ float next_up(float x) {
  const uint32_t b = __float_as_uint(x);
  if (x == INFINITY) return x;
  if (x == 0.0f) return __uint_as_float(0x00000001u);
  return __uint_as_float(x > 0.0f ? b + 1u : b - 1u);
}
}  // namespace

// One wave per work item: lanes stride over the item's points, each keeps the min / max of its world positions, then the wave
// reduces across its 64 lanes.  Min and max are exact, so the order of the reduction does not change the result (but for the sign
// of a zero, which the padding below cannot see).
__global__ void __launch_bounds__(kBoxBlock) k_instance_box_partials(const InstanceBoxItem* __restrict__ items, uint32_t n_items,
                                                                     const float4* __restrict__ points, const TransformPair* __restrict__ xf,
                                                                     double* __restrict__ partial) {
  const uint32_t item = blockIdx.x * (kBoxBlock / 64u) + threadIdx.x / 64u;
  const uint32_t lane = threadIdx.x & 63u;
  if (item >= n_items) return;   // the whole wave
  const InstanceBoxItem it = items[item];
  const float* M = xf[it.transform].o2w;
  double m[12];   // rows 0..2 of the column-major o2w, column by column
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) m[3 * c + k] = (double)M[4 * c + k];
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (uint32_t p = it.first + lane; p < it.first + it.count; p += 64u) {
    const float4 v = points[p];
    const double x = v.x, y = v.y, z = v.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // M[k] x + M[4 + k] y + M[8 + k] z + M[12 + k], left to right, no contraction (the library builds with -ffp-contract=off)
      const double w = m[k] * x + m[3 + k] * y + m[6 + k] * z + m[9 + k];
      lo[k] = min_first(lo[k], w);
      hi[k] = max_first(hi[k], w);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min_first(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = max_first(hi[k], __shfl_xor(hi[k], off, 64));
    }
  if (lane == 0) {
    double* out = partial + 6 * (size_t)item;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out[k] = lo[k];
      out[3 + k] = hi[k];
    }
  }
}

// One wave per instance: the lanes stride over its items' partials (a mesh of millions of vertices has hundreds of items) and reduce
// across the wave, then lane 0 pads as the host rule does, in the same operation order.
__global__ void __launch_bounds__(kBoxBlock) k_instance_box_finish(uint32_t n_instances, const uint32_t* __restrict__ item_first,
                                                                   const InstanceBoxItem* __restrict__ items, const double* __restrict__ partial,
                                                                   const float4* __restrict__ mesh_lo, const float4* __restrict__ mesh_hi,
                                                                   const TransformPair* __restrict__ xf,
                                                                   float4* __restrict__ box_lo, float4* __restrict__ box_hi) {
  const uint32_t i = blockIdx.x * (kBoxBlock / 64u) + threadIdx.x / 64u;
  const uint32_t lane = threadIdx.x & 63u;
  if (i >= n_instances) return;   // the whole wave
  const uint32_t first = item_first[i], end = item_first[i + 1];
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (uint32_t j = first + lane; j < end; j += 64u)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min_first(lo[k], partial[6 * (size_t)j + k]);
      hi[k] = max_first(hi[k], partial[6 * (size_t)j + 3 + k]);
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = min_first(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = max_first(hi[k], __shfl_xor(hi[k], off, 64));
    }
  if (lane != 0) return;
  const InstanceBoxItem it = items[first];
  const float* M = xf[it.transform].o2w;
  const float4 ml = mesh_lo[it.mesh], mh = mesh_hi[it.mesh];
  const double mlo[3] = {ml.x, ml.y, ml.z}, mhi[3] = {mh.x, mh.y, mh.z};
  float l[3], h[3];
  for (int k = 0; k < 3; ++k) {
    if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0;
    const double mag = fabs((double)M[k]) * max_first(fabs(mlo[0]), fabs(mhi[0])) + fabs((double)M[4 + k]) * max_first(fabs(mlo[1]), fabs(mhi[1])) +
                       fabs((double)M[8 + k]) * max_first(fabs(mlo[2]), fabs(mhi[2])) + fabs((double)M[12 + k]);
    const double pad = 1e-5 * max_first(max_first(fabs(lo[k]), fabs(hi[k])), 1e-3) + 1e-6 * (hi[k] - lo[k]) + (__builtin_isfinite(mag) ? 4.8e-7 * mag : 0.0);
    // (never NaN: lo <= 1e300 and hi >= -1e300 even when a point is infinite, so hi - lo is never inf - inf)
    l[k] = next_down((float)(lo[k] - pad));
    h[k] = next_up((float)(hi[k] + pad));
  }
  box_lo[i] = make_float4(l[0], l[1], l[2], 0.0f);
  box_hi[i] = make_float4(h[0], h[1], h[2], 0.0f);
}

hipError_t launch_instance_boxes(hipStream_t st, uint32_t n_items, const InstanceBoxItem* items, const float4* points, const TransformPair* xf,
                                 double* partial, uint32_t n_instances, const uint32_t* item_first, const float4* mesh_lo, const float4* mesh_hi,
                                 float4* box_lo, float4* box_hi) {
  if (n_instances == 0) return hipSuccess;
  const uint32_t waves = kBoxBlock / 64u;
  hipLaunchKernelGGL(k_instance_box_partials, dim3((n_items + waves - 1) / waves), dim3(kBoxBlock), 0, st, items, n_items, points, xf, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_instance_box_finish, dim3((n_instances + waves - 1) / waves), dim3(kBoxBlock), 0, st, n_instances, item_first, items,
                     partial, mesh_lo, mesh_hi, xf, box_lo, box_hi);
  return hipGetLastError();
}

}  // namespace glz
