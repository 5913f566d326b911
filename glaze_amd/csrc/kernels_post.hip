// Post kernels for gfx950 (wave64): the first-hit pass behind the feature buffers (depth, shading normal, albedo, instance id of the
// primary ray through every pixel centre) and the edge-avoiding a-trous filter that uses them as guides (denoise.h holds the filter's
// arithmetic, shared with the host reference).  Nothing here touches the path state or the accumulators of the render kernels.
#include "denoise.h"
#include "device/path_state.h"
#include "device/shading.h"
#include "device/trace_wave.h"
#include "device/trace_wave_tl.h"
#include "launch_geometry.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// First-hit pass, part 1: the closest hit of the centre ray of every pixel, through the render kernels' traversal (trace_wave /
// trace_wave_tl with a Source and a Sink of its own, as k_debug_closest).  The rays are dealt in the tile-major order of a full-frame
// TileMap, so a wave still owns an 8 x 8 block of pixels; the records are stored row-major.
// ---------------------------------------------------------------------------------------------
struct CentreSource {
  const LaunchArgs& A;
  __device__ __forceinline__ bool load(uint32_t i, vec3& origin, vec3& direction, float& tmin, float& tmax) {
    if (i >= A.map.n_local_pixels) return false;
    const PixelId px = pixel_of(A.map, i);
    if (!px.active) return false;
    camera_ray(A, A.frame, px, 0.5f, 0.5f, origin, direction);
    tmin = 0.0001f;   // as ClosestSource
    tmax = INFINITY;
    return true;
  }
};
struct FirstHitSink {
  const LaunchArgs& A;
  float4* hit;       // row-major: t (inf = miss), u, v, leaf (bits)
  uint32_t* inst;    // row-major: RTInstance of the hit, 0xFFFFFFFF = miss
  __device__ __forceinline__ void store(uint32_t i, const HitRecord& h) {
    const PixelId px = pixel_of(A.map, i);   // only rays CentreSource handed out arrive here: inside the image
    const size_t p = (size_t)px.y * A.map.width + px.x;
    const bool is_hit = h.leaf != 0xFFFFFFFFu;
    hit[p] = make_float4(is_hit ? h.t : INFINITY, h.u, h.v, __uint_as_float(h.leaf));
    inst[p] = is_hit ? (A.scene.two_level ? h.inst : A.scene.bvh_tris[h.leaf].instance) : 0xFFFFFFFFu;
  }
};
__global__ void __launch_bounds__(kBlock) k_first_hit(const LaunchArgs A, float4* hit, uint32_t* inst) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ uint4 s_top[kBvhTopNodes * 4];
  __shared__ float s_top_ray[9 * kBlock];
  stage_top(A.scene, s_top);
  TraceTally tally;
  CentreSource src{A};
  FirstHitSink sink{A, hit, inst};
  const uint32_t n = A.map.n_local_pixels;
  if (A.scene.two_level) trace_wave_tl<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
  else trace_wave<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
}

// ---------------------------------------------------------------------------------------------
// First-hit pass, part 2: the attributes, one thread per pixel (row-major).  The first lines of shade_pixel_body up to
// fetch_material_textures restated -- same operations, same order -- with texture level 0 always (kNoLod).
//   aov0 = (normal.xyz, depth)   aov1 = (albedo.rgb, instance bits)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_first_hit_attributes(const LaunchArgs A, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                                                 float4* __restrict__ aov0, float4* __restrict__ aov1) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.map.width * A.map.height) return;
  const float4 hr = hit[p];
  const uint32_t leaf = __float_as_uint(hr.w);
  if (leaf == 0xFFFFFFFFu) {
    aov0[p] = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
    aov1[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0xFFFFFFFFu));
    return;
  }
  DeviceScene S = A.scene;
  S.tex_counter = nullptr;
  PixelId px;
  px.x = p % A.map.width;
  px.y = p / A.map.width;
  px.active = true;
  vec3 origin, direction;
  camera_ray(A, A.frame, px, 0.5f, 0.5f, origin, direction);   // the ray k_first_hit traced, bit for bit
  const uint32_t hit_inst = inst[p];
  const float4* rec = S.shade_tris + 8u * (size_t)leaf;
  const float4 va0 = rec[0], va1 = rec[1], vb0 = rec[2], vb1 = rec[3], vc0 = rec[4], vc1 = rec[5], dn = rec[6], du = rec[7];
  uint32_t material_id = __float_as_uint(dn.w), xf_bits = __float_as_uint(du.w);
  if (S.two_level) {
    const RTInstance in = S.instances[hit_inst];
    material_id = in.material_id;
    xf_bits = in.transform_id | (S.xf_identity[in.transform_id] ? 0x80000000u : 0u);
  }
  const float b0 = 1.0f - hr.y - hr.z, b1 = hr.y, b2 = hr.z;
  const vec2 uv = vec2{(va1.z * b0 + vb1.z * b1) + vc1.z * b2, (va1.w * b0 + vb1.w * b1) + vc1.w * b2};
  vec3 ng = mk3(dn.x, dn.y, dn.z), dpdu = mk3(du.x, du.y, du.z);
  vec3 ns = (mk3(va0.w, va1.x, va1.y) * b0 + mk3(vb0.w, vb1.x, vb1.y) * b1) + mk3(vc0.w, vc1.x, vc1.y) * b2;
  const MatScalars mat = load_material(&S.materials[material_id]);
  const TexFootprint fp{kNoLod, 0.0f, 0.0f, 1u};
  if (mat.normal != 0) {
    const vec4 tx = texture2d_lod(S, mat.normal, uv.x, uv.y, fp);
    Frame old;
    old.s = normalize3(dpdu);
    old.n = ns;
    old.t = normalize3(cross3(old.n, old.s));
    ns = normalize3(to_world(mk3(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f), old));
    ns = ns * gl_sign(dot3(ng, ns));
  }
  if (!(xf_bits >> 31)) {
    const float4* xq = reinterpret_cast<const float4*>(&S.transforms[xf_bits & 0x7FFFFFFFu]);
    const float4 w0 = xq[4], w1 = xq[5], w2 = xq[6];
    const float w2o[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    ns = xform_tdir(w2o, ns);
  }
  vec3 n = normalize3(ns);
  if (dot3(n, direction) > 0.0f) n = -n;
  if (!(post::finite1(n.x) && post::finite1(n.y) && post::finite1(n.z))) n = mk3(0.0f, 0.0f, 0.0f);   // a zero-length ns normalises to NaN
  vec3 albedo = mk3(1.0f, 1.0f, 1.0f);
  if (mat.bsdf_index == kBsdfLambert || mat.bsdf_index == kBsdfUber) {
    const vec4 tx = texture2d_lod(S, mat.diffuse, uv.x, uv.y, fp);
    albedo = mk3(tx.x, tx.y, tx.z) * mk3(mat.diffuse_mul[0], mat.diffuse_mul[1], mat.diffuse_mul[2]);
  }
  aov0[p] = make_float4(n.x, n.y, n.z, hr.x);
  aov1[p] = make_float4(albedo.x, albedo.y, albedo.z, __uint_as_float(hit_inst));
}

// camera_ray() of every pixel at one sub-pixel offset (row-major, 3 floats each): the parity hook behind glz_debug_camera_rays
__global__ void __launch_bounds__(kBlock) k_camera_rays(const LaunchArgs A, float off_x, float off_y, float* __restrict__ o3, float* __restrict__ d3) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.map.width * A.map.height) return;
  PixelId px;
  px.x = p % A.map.width;
  px.y = p / A.map.width;
  px.active = true;
  vec3 o, d;
  camera_ray(A, A.frame, px, off_x, off_y, o, d);
  o3[3 * (size_t)p] = o.x; o3[3 * (size_t)p + 1] = o.y; o3[3 * (size_t)p + 2] = o.z;
  d3[3 * (size_t)p] = d.x; d3[3 * (size_t)p + 1] = d.y; d3[3 * (size_t)p + 2] = d.z;
}

// ---------------------------------------------------------------------------------------------
// The a-trous filter.  One thread per pixel, a wave on 64 consecutive pixels of a row, a block on a 64 x 4 patch: every tap row a wave
// reads is one coalesced 1 KiB line per plane, and at the small strides the four rows of a block share most of theirs through L1.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kPostTileW = 64, kPostTileH = kBlock / 64;
__global__ void __launch_bounds__(kBlock) k_demodulate(uint32_t n, const float4* __restrict__ result, const float4* __restrict__ aov1, float eps_albedo,
                                                       float4* __restrict__ out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  out[p] = post::demodulate(result[p], aov1[p], eps_albedo);
}
// LAST: the pass that also re-modulates (out = i_K * max(albedo, eps_a))
template <bool LAST>
__global__ void __launch_bounds__(kBlock) k_atrous(uint32_t w, uint32_t h, uint32_t k, const glz_denoise_params P, const float4* __restrict__ in,
                                                   const float4* __restrict__ aov0, const float4* __restrict__ aov1, float4* __restrict__ out) {
  const uint32_t x = blockIdx.x * kPostTileW + (threadIdx.x & 63u), y = blockIdx.y * kPostTileH + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  float4 v = post::atrous_pixel(in, aov0, w, h, x, y, k, P);
  const size_t p = (size_t)y * w + x;
  if (LAST) v = post::remodulate(v, aov1[p], P.eps_albedo);
  out[p] = v;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// blocks of k_first_hit's persistent grid (the render tracers' residency rule)
uint32_t first_hit_grid_blocks(uint32_t n_rays) { return persistent_grid(k_first_hit, n_rays).x; }
hipError_t launch_first_hit(hipStream_t st, const LaunchArgs& a, uint32_t blocks, float4* hit, uint32_t* inst) {
  if (a.map.n_local_pixels == 0) return hipSuccess;
  if (a.map.rank != 0 || a.map.world != 1) return hipErrorInvalidValue;   // the full frame: the sink stores every pixel of the image
  if (blocks == 0 || (uint64_t)blocks * kBlock > (uint64_t)a.map.n_local_pixels + kBlock) return hipErrorInvalidValue;   // the spill area holds one slot per lane of this bound
  hipLaunchKernelGGL(k_first_hit, dim3(blocks), dim3(kBlock), 0, st, a, hit, inst);
  return hipGetLastError();
}
hipError_t launch_first_hit_attributes(hipStream_t st, const LaunchArgs& a, const float4* hit, const uint32_t* inst, float4* aov0, float4* aov1) {
  const uint32_t n = a.map.width * a.map.height;
  return launch_per_item(st, k_first_hit_attributes, n, a, hit, inst, aov0, aov1);
}
hipError_t launch_camera_rays(hipStream_t st, const LaunchArgs& a, float off_x, float off_y, float* origins3, float* dirs3) {
  const uint32_t n = a.map.width * a.map.height;
  return launch_per_item(st, k_camera_rays, n, a, off_x, off_y, origins3, dirs3);
}
hipError_t launch_denoise(hipStream_t st, uint32_t w, uint32_t h, const glz_denoise_params& P, const float4* result, const float4* aov0, const float4* aov1,
                          float4* ping, float4* pong, float4* out, hipEvent_t* marks) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!post::denoise_params_valid(P) || (uint64_t)w * h > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint32_t n = w * h;
  if (marks) (void)hipEventRecord(marks[0], st);
  hipLaunchKernelGGL(k_demodulate, grid_for(n), dim3(kBlock), 0, st, n, result, aov1, P.eps_albedo, ping);
  if (marks) (void)hipEventRecord(marks[1], st);
  const dim3 grid((w + kPostTileW - 1) / kPostTileW, (h + kPostTileH - 1) / kPostTileH);
  const float4* src = ping;
  for (uint32_t k = 0; k < P.iterations; ++k) {
    const bool last = k + 1 == P.iterations;
    float4* dst = last ? out : (src == ping ? pong : ping);
    if (last) hipLaunchKernelGGL(k_atrous<true>, grid, dim3(kBlock), 0, st, w, h, k, P, src, aov0, aov1, dst);
    else hipLaunchKernelGGL(k_atrous<false>, grid, dim3(kBlock), 0, st, w, h, k, P, src, aov0, aov1, dst);
    if (marks) (void)hipEventRecord(marks[2 + k], st);
    src = dst;
  }
  return hipGetLastError();
}

}  // namespace glz
