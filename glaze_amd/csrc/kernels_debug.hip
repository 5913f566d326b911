// Debug / parity kernels behind the glz_debug_* entry points (abi_debug.cpp): arbitrary rays through the render kernels' traversal
// code, and the texture sampler, the deterministic math and the shading routines one call at a time.  Built with kernels_render.hip's
// flags (Makefile), so that the traversal inside k_debug_closest / k_debug_any is the code the render kernels run.
#include "device/shading.h"
#include "device/trace_wave.h"
#include "device/trace_wave_tl.h"
#include "launch_geometry.h"

namespace glz {
using namespace dev;

struct DebugSource {
  const float* __restrict__ o3;
  const float* __restrict__ d3;
  const float* __restrict__ tmax_arr;   // nullptr = infinity
  float tmin_all;
  __device__ __forceinline__ bool load(uint32_t i, vec3& o, vec3& d, float& tmin, float& tmax) {
    o = mk3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]);
    d = mk3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
    tmin = tmin_all;
    tmax = tmax_arr ? tmax_arr[i] : INFINITY;
    return true;
  }
};
struct DebugClosestSink {
  const DeviceScene& S;
  float* t; uint32_t* tri; uint32_t* inst; float* u; float* v;
  __device__ __forceinline__ void store(uint32_t i, const HitRecord& h) {
    const bool hit = h.leaf != 0xFFFFFFFFu;
    t[i] = hit ? h.t : INFINITY;
    tri[i] = hit ? (S.two_level ? h.world_id : S.bvh_tris[h.leaf].world_id) : 0xFFFFFFFFu;
    inst[i] = hit ? (S.two_level ? h.inst : S.bvh_tris[h.leaf].instance) : 0xFFFFFFFFu;
    u[i] = hit ? h.u : 0.0f;
    v[i] = hit ? h.v : 0.0f;
  }
};
struct DebugAnySink {
  uint8_t* out;
  __device__ __forceinline__ void store(uint32_t i, const HitRecord& h) { out[i] = h.leaf != 0xFFFFFFFFu; }
};

__global__ void __launch_bounds__(kBlock) k_debug_closest(const DeviceScene S, const float* __restrict__ o, const float* __restrict__ d, uint32_t n,
                                                          float tmin, float* t, uint32_t* tri, uint32_t* inst, float* u, float* v,
                                                          uint32_t* overflow, uint32_t overflow_depth) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ uint4 s_top[kBvhTopNodes * 4];
  __shared__ float s_top_ray[9 * kBlock];
  stage_top(S, s_top);
  TraceTally tally;
  DebugSource src{o, d, nullptr, tmin};
  DebugClosestSink sink{S, t, tri, inst, u, v};
  if (S.two_level) trace_wave_tl<false, false>(S, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, overflow, overflow_depth, n, wave_index(), wave_count(), tally);
  else trace_wave<false, false>(S, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), (LdsNodePtr)s_top, overflow, overflow_depth, n, wave_index(), wave_count(), tally);
}
__global__ void __launch_bounds__(kBlock) k_debug_any(const DeviceScene S, const float* __restrict__ o, const float* __restrict__ d,
                                                      const float* __restrict__ tmax, uint32_t n, float tmin, uint8_t* out, uint32_t* overflow,
                                                      uint32_t overflow_depth) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ uint4 s_top[kBvhTopNodes * 4];
  __shared__ float s_top_ray[9 * kBlock];
  stage_top(S, s_top);
  TraceTally tally;
  DebugSource src{o, d, tmax, tmin};
  DebugAnySink sink{out};
  if (S.two_level) trace_wave_tl<true, false>(S, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, overflow, overflow_depth, n, wave_index(), wave_count(), tally);
  else trace_wave<true, false>(S, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), (LdsNodePtr)s_top, overflow, overflow_depth, n, wave_index(), wave_count(), tally);
}

// the texture sampler on its own: n fetches of texture `id` at uv[i], level 0 (fp null: texture2d) or with the footprint fp[i] =
// (lod_base, du, dv, taps) (texture2d_lod; the caller has built the mip chain)
__global__ void __launch_bounds__(kBlock) k_debug_sample_texture(DeviceScene S, uint32_t id, const float2* __restrict__ uv, const float4* __restrict__ fp,
                                                                 uint32_t n, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  S.tex_counter = nullptr;
  const float2 c = uv[i];
  vec4 r;
  if (fp) {
    const float4 f = fp[i];
    r = texture2d_lod(S, id, c.x, c.y, TexFootprint{f.x, f.y, f.z, (uint32_t)f.w});
  } else {
    r = texture2d(S, id, c.x, c.y);
  }
  out[i] = make_float4(r.x, r.y, r.z, r.w);
}
// include/glz_detmath.h on the device; fn numbered as pyoracle.DETMATH (sin, cos, acos, atan2(y, x), log2, floor)
__global__ void __launch_bounds__(kBlock) k_debug_detmath(int fn, const float* __restrict__ x, const float* __restrict__ y, uint32_t n, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float a = x[i];
  float r;
  switch (fn) {
    case 0: r = glz_sinf(a); break;
    case 1: r = glz_cosf(a); break;
    case 2: r = glz_acosf(a); break;
    case 3: r = glz_atan2f(y[i], a); break;
    case 4: r = glz_log2f(a); break;
    default: r = glz_floorf(a); break;
  }
  out[i] = r;
}
// from_surface_color (illuminant 0) / from_illuminant_color (1) of n colours rgb3[3 i ..]: 16 bins each
__global__ void __launch_bounds__(kBlock) k_debug_color_to_spec(int illuminant, const float* __restrict__ rgb3, uint32_t n, float* __restrict__ out16) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const vec3 c = mk3(rgb3[3 * t], rgb3[3 * t + 1], rgb3[3 * t + 2]);
  const Spec s = illuminant ? from_illuminant_color(c) : from_surface_color(c);
  GLZ_BINS out16[16 * t + i] = s.w[i];
}

// The shading routines of device/shading.h one call at a time: bsdf_eval, bsdf_sample, and sample_light followed by light_emission.  The
// surface point is built the way shade_pixel builds it (woW, uv, load_material, fetch_material_textures with the level-0 footprint of a
// renderer without texture LOD), except that the frame is stored as given -- frame9 = s, t, n; null = (x, y, z) -- and not made by
// make_frame.  One uv pair serves the whole call.  Outputs start as zeros; what a routine leaves unwritten when it returns early stays zero.
__device__ __forceinline__ SurfacePoint debug_surface_point(const DeviceScene& S, uint32_t material, vec3 wo, const float* __restrict__ uv2,
                                                            const float* __restrict__ frame9) {
  SurfacePoint P;
  P.woW = wo;
  P.uv = vec2{uv2[0], uv2[1]};
  P.frame.s = frame9 ? mk3(frame9[0], frame9[1], frame9[2]) : mk3(1.0f, 0.0f, 0.0f);
  P.frame.t = frame9 ? mk3(frame9[3], frame9[4], frame9[5]) : mk3(0.0f, 1.0f, 0.0f);
  P.frame.n = frame9 ? mk3(frame9[6], frame9[7], frame9[8]) : mk3(0.0f, 0.0f, 1.0f);
  P.mat = load_material(S, material);
  fetch_material_textures(S, P, TexFootprint{kNoLod, 0.0f, 0.0f, 1u});
  return P;
}
__global__ void __launch_bounds__(kBlock) k_debug_bsdf_value(DeviceScene S, uint32_t material, const float* __restrict__ wo3, const float* __restrict__ wi3,
                                                             const float* __restrict__ uv2, const float* __restrict__ rand1, const float* __restrict__ frame9,
                                                             uint32_t n, float* __restrict__ value16, float* __restrict__ pdf) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  S.tex_counter = nullptr;
  const SurfacePoint P = debug_surface_point(S, material, mk3(wo3[3 * t], wo3[3 * t + 1], wo3[3 * t + 2]), uv2, frame9);
  Spec value = spec_set(0.0f);
  pdf[t] = bsdf_eval(S, P, mk3(wi3[3 * t], wi3[3 * t + 1], wi3[3 * t + 2]), rand1[t], value);
  GLZ_BINS value16[16 * t + i] = value.w[i];
}
__global__ void __launch_bounds__(kBlock) k_debug_bsdf_sample(DeviceScene S, uint32_t material, const float* __restrict__ wo3, const float* __restrict__ uv2,
                                                              const float* __restrict__ rand3, const float* __restrict__ frame9, uint32_t n,
                                                              float* __restrict__ wi3, float* __restrict__ value16, float* __restrict__ pdf) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  S.tex_counter = nullptr;
  const SurfacePoint P = debug_surface_point(S, material, mk3(wo3[3 * t], wo3[3 * t + 1], wo3[3 * t + 2]), uv2, frame9);
  Spec value = spec_set(0.0f);
  vec3 wi = mk3(0.0f, 0.0f, 0.0f);
  pdf[t] = bsdf_sample(S, P, mk3(rand3[3 * t], rand3[3 * t + 1], rand3[3 * t + 2]), value, wi);
  wi3[3 * t] = wi.x; wi3[3 * t + 1] = wi.y; wi3[3 * t + 2] = wi.z;
  GLZ_BINS value16[16 * t + i] = value.w[i];
}
// SKY_LDS: the sky's marginal cdf fits kSkyLdsFloats and the row search reads it, and its bracket table, from a copy in LDS made the way
// k_shade makes its own; otherwise the search reads the cdf from memory (S.sky_cdf as the host set it), all of it, as k_shade's does for a
// sky that tall.
template <bool SKY_LDS>
__global__ void __launch_bounds__(kBlock) k_debug_light_sample(DeviceScene S, uint32_t light, const float* __restrict__ pos3, const float* __restrict__ rand3,
                                                               uint32_t n, float scene_radius, float* __restrict__ wi3, float* __restrict__ dist,
                                                               float* __restrict__ pdf, float* __restrict__ emission16) {
  __shared__ uint4 s_sky[SKY_LDS ? kSkyLdsFloats / 4 + kSkyBracketFloats / 4 : 1];
  const uint16_t* bracket = nullptr;
  if (SKY_LDS) {
    static_assert(kSkyBracketFloats / 4 <= kBlock, "the bracket table is copied one piece per thread");
    const uint32_t n_sky = S.sky_header.marginal_cdf_count;   // (at most kSkyLdsFloats: launch_debug_light_sample)
    for (uint32_t i = threadIdx.x; i < (n_sky + 3u) / 4u; i += kBlock) s_sky[i] = reinterpret_cast<const uint4*>(S.sky_marginal)[i];
    if (threadIdx.x < kSkyBracketFloats / 4) s_sky[kSkyLdsFloats / 4 + threadIdx.x] = reinterpret_cast<const uint4*>(S.sky_marginal)[sky_bracket_offset(n_sky) / 4u + threadIdx.x];
    __syncthreads();
    S.sky_cdf = reinterpret_cast<const float*>(s_sky);
    bracket = reinterpret_cast<const uint16_t*>(s_sky + kSkyLdsFloats / 4);
  }
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  S.tex_counter = nullptr;
  LightSample ls;
  ls.wiW = mk3(0.0f, 0.0f, 0.0f);
  ls.pdf = 0.0f;
  ls.distance = 0.0f;
  sample_light(S, light, mk3(pos3[3 * t], pos3[3 * t + 1], pos3[3 * t + 2]), mk3(rand3[3 * t], rand3[3 * t + 1], rand3[3 * t + 2]), scene_radius, ls, bracket);
  const Spec e = light_emission(S, ls);
  wi3[3 * t] = ls.wiW.x; wi3[3 * t + 1] = ls.wiW.y; wi3[3 * t + 2] = ls.wiW.z;
  dist[t] = ls.distance;
  pdf[t] = ls.pdf;
  GLZ_BINS emission16[16 * t + i] = e.w[i];
}

hipError_t launch_debug_closest(hipStream_t st, const DeviceScene& scene, const float* o, const float* d, uint32_t n, float tmin, float* t,
                                uint32_t* tri, uint32_t* inst, float* u, float* v, uint32_t* overflow, uint32_t overflow_depth) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_debug_closest, persistent_grid(k_debug_closest, n), dim3(kBlock), 0, st, scene, o, d, n, tmin, t, tri, inst, u, v, overflow, overflow_depth);
  return hipGetLastError();
}
hipError_t launch_debug_any(hipStream_t st, const DeviceScene& scene, const float* o, const float* d, const float* tmax, uint32_t n, float tmin,
                            uint8_t* hit, uint32_t* overflow, uint32_t overflow_depth) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_debug_any, persistent_grid(k_debug_any, n), dim3(kBlock), 0, st, scene, o, d, tmax, n, tmin, hit, overflow, overflow_depth);
  return hipGetLastError();
}

hipError_t launch_debug_sample_texture(hipStream_t st, const DeviceScene& scene, uint32_t id, const float* uv2, const float* fp4, uint32_t n, float* rgba) {
  return launch_per_item(st, k_debug_sample_texture, n, scene, id, reinterpret_cast<const float2*>(uv2), reinterpret_cast<const float4*>(fp4), n,
                         reinterpret_cast<float4*>(rgba));
}
hipError_t launch_debug_detmath(hipStream_t st, int fn, const float* x, const float* y, uint32_t n, float* out) {
  return launch_per_item(st, k_debug_detmath, n, fn, x, y, n, out);
}
hipError_t launch_debug_color_to_spec(hipStream_t st, int illuminant, const float* rgb3, uint32_t n, float* out16) {
  return launch_per_item(st, k_debug_color_to_spec, n, illuminant, rgb3, n, out16);
}
hipError_t launch_debug_bsdf_value(hipStream_t st, const DeviceScene& scene, uint32_t material, const float* wo3, const float* wi3, const float* uv2,
                                   const float* rand1, const float* frame9, uint32_t n, float* value16, float* pdf) {
  return launch_per_item(st, k_debug_bsdf_value, n, scene, material, wo3, wi3, uv2, rand1, frame9, n, value16, pdf);
}
hipError_t launch_debug_bsdf_sample(hipStream_t st, const DeviceScene& scene, uint32_t material, const float* wo3, const float* uv2, const float* rand3,
                                    const float* frame9, uint32_t n, float* wi3, float* value16, float* pdf) {
  return launch_per_item(st, k_debug_bsdf_sample, n, scene, material, wo3, uv2, rand3, frame9, n, wi3, value16, pdf);
}
hipError_t launch_debug_light_sample(hipStream_t st, const DeviceScene& scene, uint32_t light, const float* pos3, const float* rand3, uint32_t n,
                                     float scene_radius, float* wi3, float* dist, float* pdf, float* emission16) {
  const bool sky_lds = scene.sky_marginal != nullptr && scene.sky_header.marginal_cdf_count > 1u && scene.sky_header.marginal_cdf_count <= kSkyLdsFloats;
  return sky_lds ? launch_per_item(st, k_debug_light_sample<true>, n, scene, light, pos3, rand3, n, scene_radius, wi3, dist, pdf, emission16)
                 : launch_per_item(st, k_debug_light_sample<false>, n, scene, light, pos3, rand3, n, scene_radius, wi3, dist, pdf, emission16);
}
}  // namespace glz
