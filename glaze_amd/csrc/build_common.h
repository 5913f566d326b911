// What the scene-build translation units (kernels_build.hip, kernels_build_sah.hip, kernels_records.hip, kernels_refit.hip) share.  Internal:
// only they include it.
#pragma once
#include <hip/hip_runtime.h>

#include "device/math.h"
#include "device/types.h"

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

// ---- the rules of a leaf, shared by the build (k_world_tris, k_leaf_boxes, k_gather_leaves) and the refit (k_refit_leaves): a refitted
// record must be the bytes a fresh build writes, so there is one definition of each ----
// world-space corners of the triangle whose three indices start at ix, under the column-major object -> world matrix M
__device__ __forceinline__ void world_triangle(const float4* vertices, const uint32_t* ix, const float* M, dev::vec3* v) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 p = vertices[2 * ix[k]];
    v[k] = dev::xform_point(M, dev::mk3(p.x, p.y, p.z));
  }
}
__device__ __forceinline__ void set_tri_vertices(BvhTri& t, const dev::vec3* v) {
  t.v0[0] = v[0].x; t.v0[1] = v[0].y; t.v0[2] = v[0].z;
  t.v1[0] = v[1].x; t.v1[1] = v[1].y; t.v1[2] = v[1].z;
  t.v2[0] = v[2].x; t.v2[1] = v[2].y; t.v2[2] = v[2].z;
}
// a triangle's box with its pad
__device__ __forceinline__ void padded_tri_box(const dev::vec3* v, float* l, float* h) {
  const float* A = &v[0].x; const float* B = &v[1].x; const float* C = &v[2].x;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    l[k] = fminf(A[k], fminf(B[k], C[k]));
    h[k] = fmaxf(A[k], fmaxf(B[k], C[k]));
    // conservative pad: the ray/triangle test may accept points a few ulps outside the exact box
    const float pad = 1e-5f * fmaxf(fmaxf(fabsf(l[k]), fabsf(h[k])), 1e-3f);
    l[k] -= pad; h[k] += pad;
  }
}
// the box of two boxes: of a pair's two triangles (first one in `a`), of a node's two children (left one in `a`)
__device__ __forceinline__ float4 union_lo(float4 a, float4 b) { return make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f); }
__device__ __forceinline__ float4 union_hi(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), 0.0f); }
// The corners of a leaf's record (types.h BvhQuad): A = (q0, q1, q2), B = (q0, q2, q3).  t: the leaf's first triangle; b: where its
// partner is, read only if there is one; fits: the partner reads (p0, p2, d); fits_swapped (kQuadSwapped, set here): it reads
// (p0, d, p1), so it is A and the first one B.
__device__ __forceinline__ void quad_corners(BvhQuad& q, const BvhTri& t, const BvhTri& b, bool fits, bool fits_swapped) {
  const float* c[4] = {t.v0, t.v1, t.v2, t.v2};   // a single triangle: q3 repeats q2 (never looked at)
  if (fits) {                    // second triangle = (p0, p2, d)
    c[3] = b.v2;
  } else if (fits_swapped) {     // second triangle = (p0, d, p1): it is A, the first one B
    c[1] = b.v1;
    c[2] = t.v1;
    c[3] = t.v2;
    q.prim_flags |= kQuadSwapped;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { q.q0[k] = c[0][k]; q.q1[k] = c[1][k]; q.q2[k] = c[2][k]; q.q3[k] = c[3][k]; }
}

// ---- the quantisation grid and the node boxes on it (k_grid_params / k_emit_nodes* of the build, k_refit_quantise) ----
constexpr float kGridReach = 1.9073486e-6f;   // 2^-19: how far past the bounds the grid reaches, as a fraction of the largest coordinate
// the grid from a root box (kernels_build.hip k_grid_params: the build's kernel, launched by the refit as well)
hipError_t launch_grid_params(hipStream_t st, const float4* root_lo, const float4* root_hi, BvhGrid* grid);

// grid coordinate of a world coordinate; the SAME expression maps the ray origin in the tracer
__device__ __forceinline__ float to_grid(float x, float lo, float inv_cell) { return (x - lo) * inv_cell; }
// `margin`: cells every box grows by on that axis beyond the 1/16 (grid_margin below)
__device__ __forceinline__ uint32_t quant_lo(float x, float lo, float inv_cell, float margin) {
  // 1/16 cell of slack covers the rounding of to_grid() at grid coordinates up to 32767 (ulp 2^-9)
  const float g = floorf(to_grid(x, lo, inv_cell) - 0.0625f - margin);
  return (uint32_t)fminf(fmaxf(g, 0.0f), (float)kBvhGridMax);
}
__device__ __forceinline__ uint32_t quant_hi(float x, float lo, float inv_cell, float margin) {
  const float g = ceilf(to_grid(x, lo, inv_cell) + 0.0625f + margin);
  return (uint32_t)fminf(fmaxf(g, 0.0f), (float)kBvhGridMax);
}
// The tracer leaves a box out when its entry distance lies behind the hit it already has, so a box's entry must not round past the
// distance of a triangle inside it: the plane distance (an fma in grid space) and the triangle's t (sheared coordinates) each carry a
// few ulps of the coordinates involved.  Where a cell is a fair fraction of the scene the 1/16 above is that margin; across the thin
// side of a FLAT scene (a floor plan: every box of no thickness, cells of 1e-13 units, the builders' relative pad nothing near
// coordinate 0) it is not, and exact ties between coincident triangles went to whichever was met first (tools/gpu_fuzz_parity.py,
// seed 61907).  So every box also grows by 2^-19 of the largest coordinate of the grid's bounds, whatever that is in cells
// (k_grid_params lets the grid reach that far past the bounds).
__device__ __forceinline__ void grid_margin(const BvhGrid& g, float* margin) {
  float largest = 0.0f;
  for (int k = 0; k < 3; ++k) largest = fmaxf(largest, fmaxf(fabsf(g.lo[k]), fabsf(g.lo[k] + (float)kBvhGridMax * g.cell[k])));
  for (int k = 0; k < 3; ++k) margin[k] = fminf((kGridReach * largest) * g.inv_cell[k], 65536.0f);
}

// the three box words of a wide node's child on the grid: one word per axis, lo | hi << 16
__device__ __forceinline__ void quant_box(float4 l, float4 h, const BvhGrid& g, const float* gm, uint32_t* w) {
  w[0] = quant_lo(l.x, g.lo[0], g.inv_cell[0], gm[0]) | (quant_hi(h.x, g.lo[0], g.inv_cell[0], gm[0]) << 16);
  w[1] = quant_lo(l.y, g.lo[1], g.inv_cell[1], gm[1]) | (quant_hi(h.y, g.lo[1], g.inv_cell[1], gm[1]) << 16);
  w[2] = quant_lo(l.z, g.lo[2], g.inv_cell[2], gm[2]) | (quant_hi(h.z, g.lo[2], g.inv_cell[2], gm[2]) << 16);
}

// The binned SAH builder on the device (kernels_build_sah.hip): fills children / parent (links >= 0 inner node, < 0 ~leaf; parent by
// box slot, leaf j at (n-1)+j) over the n >= 2 leaf boxes leaf_lo / leaf_hi, one or seven launches and one synchronisation per level.
hipError_t build_sah_levels(hipStream_t st, uint32_t n, const float4* leaf_lo, const float4* leaf_hi, int2* children, int* parent);

}  // namespace glz
