// The edge-avoiding a-trous filter of glz_denoise_params and the firefly rejection of glz_despeckle_params (include/glaze_abi.h holds the
// specifications), one pixel of one pass, in the
// ONE form both the host reference (glz_host_denoise, g++) and the device kernels (kernels_post.hip, hipcc) compile: the same operations
// in the same order, -ffp-contract=off and correctly rounded divisions on both sides, so the two agree bit for bit.  Only + - * /,
// comparisons and selects; no library function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glaze_abi.h"

#if defined(__HIPCC__)
#define GLZ_POST_FN __host__ __device__ __forceinline__
#else
#define GLZ_POST_FN inline
#endif

namespace glz {
namespace post {

constexpr uint32_t kDenoiseMaxIterations = GLZ_DENOISE_MAX_ITERATIONS;
inline glz_denoise_params denoise_defaults() { return glz_denoise_params{5u, 4.0f, 1.0f, 6u, 1.0f / 256.0f, 1e-3f, 1e-8f}; }
// iterations in 1 .. 8, finite positive sigmas, at most 31 squarings of the normal weight (the trip count of a loop in every tap of every
// pixel: it must be bounded before a kernel is launched with it); the epsilons are taken as they are
inline bool denoise_params_valid(const glz_denoise_params& p) {
  return p.iterations >= 1u && p.iterations <= kDenoiseMaxIterations && p.sigma_color > 0.0f && p.sigma_color <= 3.4e38f && p.sigma_depth > 0.0f &&
         p.sigma_depth <= 3.4e38f && p.normal_power_log2 <= GLZ_DENOISE_MAX_NORMAL_POWER_LOG2;
}
constexpr const char* kDenoiseParamsMessage = "denoise: iterations must be 1 .. 8, sigma_color and sigma_depth finite and positive, normal_power_log2 at most 31";

GLZ_POST_FN bool finite1(float v) { return (v < 0.0f ? -v : v) <= 3.4028234663852886e38f; }   // false for NaN and the infinities
GLZ_POST_FN bool finite3(float4 v) { return finite1(v.x) && finite1(v.y) && finite1(v.z); }
GLZ_POST_FN float abs1(float v) { return v < 0.0f ? -v : v; }

// max(albedo, eps_a) per channel (a NaN albedo counts as eps_a)
GLZ_POST_FN float4 clamped_albedo(float4 a, float eps) { return make_float4(a.x > eps ? a.x : eps, a.y > eps ? a.y : eps, a.z > eps ? a.z : eps, a.w); }
// i_0 = c / max(albedo, eps_a); .w passes through
GLZ_POST_FN float4 demodulate(float4 c, float4 albedo, float eps) {
  const float4 a = clamped_albedo(albedo, eps);
  return make_float4(c.x / a.x, c.y / a.y, c.z / a.z, c.w);
}

// h = (1/16, 1/4, 3/8, 1/4, 1/16) at offset d in -2 .. 2
GLZ_POST_FN float tap_weight(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// One axis of g(p): z0 = depth at p (finite), zf / zb = depth of the next / previous pixel on the axis (has_* false at the image border).
// The forward or the backward difference, whichever is finite and smaller in magnitude (the forward one on a tie); 0 if neither is finite.
GLZ_POST_FN float depth_slope(float z0, bool has_f, float zf, bool has_b, float zb) {
  const float df = zf - z0, db = z0 - zb;
  const bool okf = has_f && finite1(df), okb = has_b && finite1(db);
  if (okf && okb) return abs1(db) < abs1(df) ? db : df;
  return okf ? df : (okb ? db : 0.0f);
}

// i_{k+1}(p) of pixel (x, y): `in` = i_k, aov0 = (normal.xyz, depth), both w * h row-major.  Taps row by row (dy outer, dx inner), sums in
// that order.  The returned .w is in(p).w.
GLZ_POST_FN float4 atrous_pixel(const float4* __restrict__ in, const float4* __restrict__ aov0, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t k,
                           const glz_denoise_params& P) {
  const int s = 1 << k;
  const float sigma_k = P.sigma_color * (1.0f / (float)(1u << k));
  const float sk2 = sigma_k * sigma_k;
  const size_t ip = (size_t)y * w + x;
  const float4 cp = in[ip], gp = aov0[ip];
  const bool fin_p = finite3(cp), hit_p = finite1(gp.w);
  const float px = fin_p ? cp.x : 0.0f, py = fin_p ? cp.y : 0.0f, pz = fin_p ? cp.z : 0.0f;
  const float np2 = (px * px + py * py) + pz * pz;
  float gx = 0.0f, gy = 0.0f;
  if (hit_p) {
    gx = depth_slope(gp.w, x + 1u < w, x + 1u < w ? aov0[ip + 1].w : 0.0f, x > 0u, x > 0u ? aov0[ip - 1].w : 0.0f);
    gy = depth_slope(gp.w, y + 1u < h, y + 1u < h ? aov0[ip + w].w : 0.0f, y > 0u, y > 0u ? aov0[ip - w].w : 0.0f);
  }
  const float zscale = P.eps_depth * gp.w;
  float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = (int)y + s * dy;
    if (qy < 0 || qy >= (int)h) continue;
    // the row's five taps of both planes are requested before any of them is used: ten loads in flight instead of one dependent round
    // trip per tap (an x outside the image reads the clamped column and is dropped below)
    float4 cqs[5], gqs[5];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = (int)x + s * dx;
      const size_t iq = (size_t)qy * w + (size_t)(qx < 0 ? 0 : (qx >= (int)w ? (int)w - 1 : qx));
      cqs[dx + 2] = in[iq];
      gqs[dx + 2] = aov0[iq];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = (int)x + s * dx;
      if (qx < 0 || qx >= (int)w) continue;
      const float4 cq = cqs[dx + 2];
      if (!finite3(cq)) continue;
      float wt = 1.0f;
      if (dx != 0 || dy != 0) {
        const float4 gq = gqs[dx + 2];
        const bool hit_q = finite1(gq.w);
        if (hit_q != hit_p) continue;
        const float ex = cq.x - px, ey = cq.y - py, ez = cq.z - pz;
        const float d2 = (ex * ex + ey * ey) + ez * ez;
        const float nq2 = (cq.x * cq.x + cq.y * cq.y) + cq.z * cq.z;
        // every weight is a ratio; the tap's product of them is formed as ONE quotient (a correctly rounded division is ten instructions)
        const float cn = sk2 * ((np2 + nq2) + P.eps_color), cd = cn + d2;   // w_c = cn / cd
        if (hit_p) {
          const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
          float wn = dn > 0.0f ? dn : 0.0f;
          for (uint32_t j = 0; j < P.normal_power_log2; ++j) wn = wn * wn;
          const float ax = (float)(s * dx) * gx, ay = (float)(s * dy) * gy;
          const float a = (gq.w - gp.w) - (ax + ay), b = P.sigma_depth * ((abs1(ax) + abs1(ay)) + zscale);
          const float zn = b * b, zd = zn + a * a;                          // w_z = zn / zd
          wt = (wn * (cn * zn)) / (cd * zd);
        } else {
          wt = cn / cd;
        }
        if (!(wt > 0.0f)) continue;   // zero, or NaN out of degenerate guides: the tap does not count
      }
      const float hw = (tap_weight(dy) * tap_weight(dx)) * wt;
      sw = sw + hw;
      sx = sx + hw * cq.x;
      sy = sy + hw * cq.y;
      sz = sz + hw * cq.z;
    }
  }
  if (!(sw > 0.0f)) return cp;
  return make_float4(sx / sw, sy / sw, sz / sw, cp.w);
}

// out(p).rgb = i_K(p) * max(albedo(p), eps_a)
GLZ_POST_FN float4 remodulate(float4 i, float4 albedo, float eps) {
  const float4 a = clamped_albedo(albedo, eps);
  return make_float4(i.x * a.x, i.y * a.y, i.z * a.z, i.w);
}

// ---- firefly rejection (glz_despeckle_params; include/glaze_abi.h holds the specification) ----------------------------------------
inline glz_despeckle_params despeckle_defaults() { return glz_despeckle_params{2u, 2u, 8.0f}; }
// radius 1 or 2 (the window unrolls: a template parameter of the kernel), trim 0 .. 3 (the sorted top-4), ratio finite and >= 1
inline bool despeckle_params_valid(const glz_despeckle_params& p) {
  return (p.radius == 1u || p.radius == 2u) && p.trim <= GLZ_DESPECKLE_MAX_TRIM && p.ratio >= 1.0f && p.ratio <= 3.4e38f;
}
constexpr const char* kDespeckleParamsMessage = "despeckle: radius must be 1 or 2, trim 0 .. 3, ratio finite and at least 1";

// i_0'(p) of pixel (x, y): `in` = i_0, aov0 = (normal.xyz, depth), both w * h row-major.  The window row by row (dy outer, dx inner); its
// L values stay in `l` (-inf where q is not usable: such an entry can never displace one of the m > trim real ones from the top
// trim + 1, and `use` keeps it out of the sum).  M comes from a sorted top-4 kept by compare and select.
template <int RADIUS>
GLZ_POST_FN float4 despeckle_pixel(const float4* __restrict__ in, const float4* __restrict__ aov0, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t trim,
                                   float ratio) {
  constexpr int kSide = 2 * RADIUS + 1;
  constexpr float kLowest = -__builtin_huge_valf();
  const size_t ip = (size_t)y * w + x;
  const float4 cp = in[ip];
  if (!(finite1(aov0[ip].w) && finite3(cp))) return cp;   // not a candidate
  float l[kSide * kSide];
  bool use[kSide * kSide];
  float t0 = kLowest, t1 = kLowest, t2 = kLowest, t3 = kLowest;   // the four largest, t0 >= t1 >= t2 >= t3
  uint32_t m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -RADIUS; dy <= RADIUS; ++dy) {
    const int qy = (int)y + dy;
    const bool row_in = qy >= 0 && qy < (int)h;
    const size_t row = (size_t)(row_in ? qy : (int)y) * w;   // (a row outside the image reads the pixel's own and is dropped below)
    // the row's values of both planes are requested before any of them is used (an x outside the image reads the clamped column)
    float4 cqs[kSide];
    float zqs[kSide];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
      const int qx = (int)x + dx;
      const size_t iq = row + (size_t)(qx < 0 ? 0 : (qx >= (int)w ? (int)w - 1 : qx));
      cqs[dx + RADIUS] = in[iq];
      zqs[dx + RADIUS] = aov0[iq].w;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -RADIUS; dx <= RADIUS; ++dx) {
      const int qx = (int)x + dx;
      const float4 cq = cqs[dx + RADIUS];
      const bool ok = row_in && qx >= 0 && qx < (int)w && (dx != 0 || dy != 0) && finite1(zqs[dx + RADIUS]) && finite3(cq);
      float v = ok ? (cq.x + cq.y) + cq.z : kLowest;
      const int i = (dy + RADIUS) * kSide + (dx + RADIUS);
      l[i] = v;
      use[i] = ok;
      m += ok ? 1u : 0u;
      // insert v into the sorted four: at each place the larger stays, the smaller moves on
      float hi;
      hi = v > t0 ? v : t0; v = v > t0 ? t0 : v; t0 = hi;
      hi = v > t1 ? v : t1; v = v > t1 ? t1 : v; t1 = hi;
      hi = v > t2 ? v : t2; v = v > t2 ? t2 : v; t2 = hi;
      t3 = v > t3 ? v : t3;
    }
  }
  if (m <= trim) return cp;
  const float M = trim == 0u ? t0 : (trim == 1u ? t1 : (trim == 2u ? t2 : t3));
  float sum = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < kSide * kSide; ++i) {
    const float v = l[i] < M ? l[i] : M;
    sum = use[i] ? sum + v : sum;
  }
  const float mu = sum / (float)m;
  const float T = ratio * mu;
  const float lp = (cp.x + cp.y) + cp.z;
  if (!(T >= 0.0f && lp > T)) return cp;
  const float f = T / lp;
  return make_float4(cp.x * f, cp.y * f, cp.z * f, cp.w);
}

// the whole filter on host arrays (denoise_host.cpp); P must be valid, out must not overlap an input
void host_denoise(uint32_t w, uint32_t h, const float4* result, const float4* aov0, const float4* aov1, const glz_denoise_params& P, float4* out);
// the rejection of D on the demodulated image, then either out = i_0' * A (with_filter false: only P.eps_albedo is used) or the filter's
// passes on i_0' -- the composition read_denoised runs when the rejection is enabled.  D and P must be valid, out must not overlap an input
void host_despeckle(uint32_t w, uint32_t h, const float4* result, const float4* aov0, const float4* aov1, const glz_despeckle_params& D,
                    const glz_denoise_params& P, bool with_filter, float4* out);

}  // namespace post
}  // namespace glz
