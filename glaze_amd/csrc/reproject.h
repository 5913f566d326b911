// Motion vectors and history reprojection (glz_renderer_read_motion, glz_renderer_reproject; include/glaze_abi.h holds the specification):
// the forward projection of a world point and one pixel of the reprojection rule, in the ONE form both the host references
// (glz_host_project_points, glz_host_reproject; g++) and the device kernels (kernels_post.hip; hipcc) compile: the same operations in the
// same order, -ffp-contract=off and correctly rounded divisions and square roots on both sides, so the two agree bit for bit.  Only
// + - * /, comparisons, selects, glz_floorf and one sqrt.
#pragma once
#include "denoise.h"
#include "glz_detmath.h"

namespace glz {
namespace post {

inline glz_reproject_params reproject_defaults() { return glz_reproject_params{1.0f / 64.0f}; }
inline bool reproject_params_valid(const glz_reproject_params& p) { return p.depth_tolerance > 0.0f && p.depth_tolerance <= 3.4e38f; }
constexpr const char* kReprojectParamsMessage = "reproject: depth_tolerance must be finite and positive";

// glz_host_project_constants' 32 floats and the camera type: what a kernel is handed by value
struct ProjectConstants {
  float world2camera[16], camera2screen[16];   // column-major
  uint32_t persp;
};

struct Projected {
  float fx, fy, z;   // invalid: (0, 0, +inf)
};
// project_point of the specification
GLZ_POST_FN Projected project_point(const ProjectConstants& C, float w, float h, float x, float y, float z) {
  const float* m = C.world2camera;
  const float* p = C.camera2screen;
  const float cx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
  const float cy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
  const float cz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
  float nx = cx, ny = cy, zz = -cz;
  bool front = true;
  if (C.persp != 0u) {
    const float d = -cz;
    front = d > 0.0f;
    nx = (((p[0] * cx + p[4] * cy) + p[8] * cz) + p[12]) / d;
    ny = (((p[1] * cx + p[5] * cy) + p[9] * cz) + p[13]) / d;
    zz = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
  }
  const float fx = ((nx + 1.0f) * 0.5f) * w, fy = ((ny + 1.0f) * 0.5f) * h;
  const bool valid = front && finite1(zz) && zz > 0.0f && finite1(fx) && finite1(fy);
  Projected r;
  r.fx = valid ? fx : 0.0f;
  r.fy = valid ? fy : 0.0f;
  r.z = valid ? zz : __builtin_huge_valf();
  return r;
}

// The motion plane's value of pixel (px, py) whose first hit lies at the world point (x, y, z) in the PREVIOUS state and carries `bits`
GLZ_POST_FN float4 motion_value(const ProjectConstants& C, uint32_t w, uint32_t h, uint32_t px, uint32_t py, float x, float y, float z, float bits) {
  const Projected r = project_point(C, (float)w, (float)h, x, y, z);
  if (!finite1(r.z)) return make_float4(0.0f, 0.0f, __builtin_huge_valf(), bits);
  return make_float4(r.fx - ((float)px + 0.5f), r.fy - ((float)py + 0.5f), r.z, bits);
}

GLZ_POST_FN uint32_t float_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}
// floor(q) = p + floor(m) as a tap coordinate: a motion that is not finite, or so large that no tap can be inside, gives -2 (both taps outside)
GLZ_POST_FN int tap_origin(float floor_m, uint32_t p, uint32_t size) {
  const float reach = (float)size + 2.0f;
  return (floor_m >= -reach && floor_m <= reach) ? (int)p + (int)floor_m : -2;
}
GLZ_POST_FN size_t clamped(int v, uint32_t size) { return (size_t)(v < 0 ? 0 : (v >= (int)size ? (int)size - 1 : v)); }

// out(p) of pixel (x, y): motion, color, aov0 = (normal.xyz, depth), aov1 = (albedo.rgb, instance bits), all w * h row-major, the last
// three of the PREVIOUS frame.  Every value the four taps need -- four colours, four instance words, the twelve depths of the 4 x 4 block
// without its corners -- is requested before the first is used (a coordinate outside the image reads the clamped one and is dropped).
GLZ_POST_FN float4 reproject_pixel(const float4* __restrict__ motion, const float4* __restrict__ color, const float4* __restrict__ aov0,
                                   const float4* __restrict__ aov1, uint32_t w, uint32_t h, uint32_t x, uint32_t y, float tolerance) {
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 m = motion[(size_t)y * w + x];
  const float zp = m.z;
  if (!finite1(zp)) return zero;
  // q = p + m: its integer part is p + floor(m) and its fraction that of m, both exact
  const float fmx = glz_floorf(m.x), fmy = glz_floorf(m.y);
  const float ax = m.x - fmx, ay = m.y - fmy;
  const int x0 = tap_origin(fmx, x, w), y0 = tap_origin(fmy, y, h);
  size_t col[4], row[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 4; ++i) {
    col[i] = clamped(x0 - 1 + i, w);
    row[i] = clamped(y0 - 1 + i, h) * w;
  }
  float4 c[4];
  float id[4], z[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 4; ++t) {
    const size_t i = row[1 + (t >> 1)] + col[1 + (t & 1)];
    c[t] = color[i];
    id[t] = aov1[i].w;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 16; ++i) {
    const int r = i >> 2, k = i & 3;
    z[i] = ((r == 0 || r == 3) && (k == 0 || k == 3)) ? 0.0f : aov0[row[r] + col[k]].w;
  }
  const uint32_t want = float_bits(m.w);
  float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int t = 0; t < 4; ++t) {
    const int dx = t & 1, dy = t >> 1;
    const int tx = x0 + dx, ty = y0 + dy;
    const float wt = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
    const bool inside = tx >= 0 && tx < (int)w && ty >= 0 && ty < (int)h;
    const int r = 1 + dy, k = 1 + dx;
    const float zt = z[4 * r + k];
    const float gx = depth_slope(zt, tx + 1 < (int)w, z[4 * r + k + 1], tx > 0, z[4 * r + k - 1]);
    const float gy = depth_slope(zt, ty + 1 < (int)h, z[4 * (r + 1) + k], ty > 0, z[4 * (r - 1) + k]);
    const float zh = zt + (gx * (ax - (float)dx) + gy * (ay - (float)dy));
    const bool ok = inside && float_bits(id[t]) == want && finite3(c[t]) && abs1(zh - zp) <= tolerance * zp;
    if (ok) {
      sw = sw + wt;
      sx = sx + wt * c[t].x;
      sy = sy + wt * c[t].y;
      sz = sz + wt * c[t].z;
    }
  }
  if (!(sw > 0.0f)) return zero;
  return make_float4(sx / sw, sy / sw, sz / sw, sw);
}

// the references on host arrays (denoise_host.cpp); P must be valid, out must not overlap an input
void host_project_points(const ProjectConstants& C, uint32_t w, uint32_t h, const float* points3, size_t n, float* out3);
void host_reproject(uint32_t w, uint32_t h, const float4* motion, const float4* color, const float4* aov0, const float4* aov1, const glz_reproject_params& P,
                    float4* out);

}  // namespace post
}  // namespace glz
