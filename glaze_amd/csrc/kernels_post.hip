// Post kernels for gfx950 (wave64): the first-hit pass behind the feature buffers (depth, shading normal, albedo, instance id of the
// primary ray through every pixel centre) and the edge-avoiding a-trous filter that uses them as guides (denoise.h holds the filter's
// arithmetic, shared with the host reference).  Nothing here touches the path state or the accumulators of the render kernels.
#include "denoise.h"
#include "device/hit_vertex.h"
#include "device/path_state.h"
#include "device/shading.h"
#include "device/trace_wave.h"
#include "device/trace_wave_tl.h"
#include "launch_geometry.h"
#include "reproject.h"

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
// What the post tracers store per ray: hit = (t (inf = miss), u, v, leaf bits), inst = the RTInstance of the hit (0xFFFFFFFF = miss).
// BY_PIXEL: at the ray's pixel, row-major (k_first_hit); otherwise at the ray's slot in its list (k_guide_trace).
template <bool BY_PIXEL>
struct HitSink {
  const LaunchArgs& A;
  float4* hit;
  uint32_t* inst;
  __device__ __forceinline__ void store(uint32_t i, const HitRecord& h) {
    const PixelId px = pixel_of(A.map, i);   // (BY_PIXEL) only rays CentreSource handed out arrive here: inside the image
    const size_t p = BY_PIXEL ? (size_t)px.y * A.map.width + px.x : i;
    const bool is_hit = h.leaf != 0xFFFFFFFFu;
    hit[p] = pack_hit(h);
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
  HitSink<true> sink{A, hit, inst};
  const uint32_t n = A.map.n_local_pixels;
  if (A.scene.two_level) trace_wave_tl<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
  else trace_wave<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
}

// ---------------------------------------------------------------------------------------------
// One vertex of a guide chain: the hit vertex of shade_pixel_body (device/hit_vertex.h) with texture level 0 always (kNoLod).  Gives the
// vertex's planes' values (the normal turned against `direction`, the albedo) and, with CHAIN, the ray the path would go on with through
// a specular material: `point` and `wiW` as shade_pixel_body forms them (bsdf_sample with xi = (0, 0, 1 - 2^-24): Mirror ignores it,
// Glass takes the transmitted branch unless its Fresnel term is 1).
// ---------------------------------------------------------------------------------------------
struct GuideVertex {
  vec3 n, albedo;
  bool go_on;        // CHAIN: the material is specular and bsdf_sample gave a direction to follow
  vec3 point, wiW;   // CHAIN, go_on: the next segment
};
template <bool CHAIN>
__device__ __forceinline__ GuideVertex guide_vertex(const DeviceScene& S, float4 hr, uint32_t hit_inst, vec3 direction) {
  const TexFootprint fp{kNoLod, 0.0f, 0.0f, 1u};
  HitVertex hv = load_hit_vertex(S, hr, [&]() { return hit_inst; });
  finish_hit_vertex<CHAIN, false>(S, hv, fp);   // (false, here and below: the sampler without the shading kernels' short forms, device/shading.h texel_address)
  const MatScalars& mat = hv.mat;
  GuideVertex v;
  v.n = normalize3(hv.ns);
  if (dot3(v.n, direction) > 0.0f) v.n = -v.n;
  if (!(post::finite1(v.n.x) && post::finite1(v.n.y) && post::finite1(v.n.z))) v.n = mk3(0.0f, 0.0f, 0.0f);   // a zero-length ns normalises to NaN
  v.albedo = mk3(1.0f, 1.0f, 1.0f);
  if (mat.bsdf_index == kBsdfLambert || mat.bsdf_index == kBsdfUber) {
    const vec4 tx = texture2d_lod<false>(S, mat.diffuse, hv.uv.x, hv.uv.y, fp);
    v.albedo = mk3(tx.x, tx.y, tx.z) * mk3(mat.diffuse_mul[0], mat.diffuse_mul[1], mat.diffuse_mul[2]);
  }
  v.go_on = false;
  v.point = hv.point;
  v.wiW = mk3(0.0f, 0.0f, 0.0f);
  if (CHAIN && mat.is_specular != 0) {
    const SurfacePoint P = hit_surface_point<false>(S, hv, direction, fp);
    Spec value = spec_set(0.0f);
    const float pdf = bsdf_sample(S, P, mk3(0.0f, 0.0f, 0x1.fffffep-1f), value, v.wiW);
    v.go_on = pdf != 0.0f && post::finite1(v.wiW.x) && post::finite1(v.wiW.y) && post::finite1(v.wiW.z);
  }
  return v;
}

// ---------------------------------------------------------------------------------------------
// First-hit pass, part 2: the attributes of the first vertex, one thread per pixel (row-major).
//   aov0 = (normal.xyz, depth)   aov1 = (albedo.rgb, instance bits)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_miss_planes(float4* __restrict__ aov0, float4* __restrict__ aov1, uint32_t p) {
  aov0[p] = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
  aov1[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0xFFFFFFFFu));
}
__device__ __forceinline__ vec3 centre_ray_direction(const LaunchArgs& A, uint32_t p) {
  PixelId px;
  px.x = p % A.map.width;
  px.y = p / A.map.width;
  px.active = true;
  vec3 origin, direction;
  camera_ray(A, A.frame, px, 0.5f, 0.5f, origin, direction);   // the ray k_first_hit traced, bit for bit
  return direction;
}
__global__ void __launch_bounds__(kBlock) k_first_hit_attributes(const LaunchArgs A, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                                                 float4* __restrict__ aov0, float4* __restrict__ aov1) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.map.width * A.map.height) return;
  const float4 hr = hit[p];
  if (__float_as_uint(hr.w) == 0xFFFFFFFFu) {
    store_miss_planes(aov0, aov1, p);
    return;
  }
  DeviceScene S = A.scene;
  S.tex_counter = nullptr;
  const uint32_t hit_inst = inst[p];
  const GuideVertex v = guide_vertex<false>(S, hr, hit_inst, centre_ray_direction(A, p));
  aov0[p] = make_float4(v.n.x, v.n.y, v.n.z, hr.x);
  aov1[p] = make_float4(v.albedo.x, v.albedo.y, v.albedo.z, __uint_as_float(hit_inst));
}

// ---------------------------------------------------------------------------------------------
// Through-specular guides (GLZ_GUIDE_THROUGH_SPECULAR): the chain of segments the path itself would follow through Mirror and Glass.
// Segment 0 is the centre ray (k_first_hit above); segment k >= 1 lives in a COMPACTED list of rays -- o = (origin, depth so far),
// d = (direction, pixel bits) -- with its length in device memory, so that a bounce costs what its live rays cost and the host never
// reads a count back: a kernel whose list is empty returns at once.
//   k_guide_continue<FIRST>  vertex k of every live ray: writes the vertex's planes at the ray's pixel (a later vertex overwrites them;
//                            a later segment that misses leaves them, which makes the last vertex hit the reporting one) and, where the
//                            chain goes on, appends segment k + 1 to the next list (ballot + popcount, one atomic per wave).
//   k_guide_trace            the closest hits of a list, stored at the rays' slots.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t list_slot(uint32_t* count, bool push) {
  const unsigned long long m = __ballot(push);
  uint32_t slot = 0;
  if (push) {
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  }
  return slot;
}
// vertex k of ray `i` (FIRST: of pixel i); all lanes of a wave call it together
template <bool FIRST>
__device__ __forceinline__ void guide_continue_ray(const LaunchArgs& A, const DeviceScene& S, uint32_t i, bool live, bool may_push, const float4* __restrict__ hit,
                                                   const uint32_t* __restrict__ inst, const float4* __restrict__ in_o, const float4* __restrict__ in_d,
                                                   float4* __restrict__ out_o, float4* __restrict__ out_d, uint32_t* out_count, float4* __restrict__ aov0,
                                                   float4* __restrict__ aov1) {
  bool push = false;
  uint32_t p = 0;
  float depth = 0.0f;
  vec3 point = mk3(0.0f, 0.0f, 0.0f), wiW = mk3(0.0f, 0.0f, 0.0f);
  if (live) {
    const float4 hr = hit[i];
    vec3 direction;
    float before = 0.0f;
    if (FIRST) {
      p = i;
      direction = centre_ray_direction(A, p);
    } else {
      const float4 ro = in_o[i], rd = in_d[i];
      p = __float_as_uint(rd.w);
      direction = mk3(rd.x, rd.y, rd.z);
      before = ro.w;
    }
    if (__float_as_uint(hr.w) == 0xFFFFFFFFu) {
      if (FIRST) store_miss_planes(aov0, aov1, p);   // (a later segment that misses: the planes of the vertex before stay)
    } else {
      const uint32_t hit_inst = inst[i];
      const GuideVertex v = guide_vertex<true>(S, hr, hit_inst, direction);
      depth = FIRST ? hr.x : before + hr.x;
      aov0[p] = make_float4(v.n.x, v.n.y, v.n.z, depth);
      aov1[p] = make_float4(v.albedo.x, v.albedo.y, v.albedo.z, __uint_as_float(hit_inst));
      push = may_push && v.go_on;
      point = v.point;
      wiW = v.wiW;
    }
  }
  const uint32_t slot = list_slot(out_count, push);
  if (push) {
    out_o[slot] = make_float4(point.x, point.y, point.z, depth);
    out_d[slot] = make_float4(wiW.x, wiW.y, wiW.z, __uint_as_float(p));
  }
}
// the length of a list: the same in every lane, and the compiler has to know it (trace_wave)
__device__ __forceinline__ uint32_t list_length(const uint32_t* count) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)*count); }

// vertex 0: one thread per pixel (row-major), in place of k_first_hit_attributes
__global__ void __launch_bounds__(kBlock) k_guide_first(const LaunchArgs A, const float4* __restrict__ hit, const uint32_t* __restrict__ inst, float4* __restrict__ out_o,
                                                        float4* __restrict__ out_d, uint32_t* out_count, float4* __restrict__ aov0, float4* __restrict__ aov1) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  DeviceScene S = A.scene;
  S.tex_counter = nullptr;
  guide_continue_ray<true>(A, S, p, p < A.map.width * A.map.height, true, hit, inst, nullptr, nullptr, out_o, out_d, out_count, aov0, aov1);
}
// vertex k >= 1: a persistent grid strides over the list, a block on kBlock consecutive rays at a time
__global__ void __launch_bounds__(kBlock) k_guide_continue(const LaunchArgs A, uint32_t may_push, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                                           const float4* __restrict__ in_o, const float4* __restrict__ in_d, const uint32_t* in_count,
                                                           float4* __restrict__ out_o, float4* __restrict__ out_d, uint32_t* out_count, float4* __restrict__ aov0,
                                                           float4* __restrict__ aov1) {
  const uint32_t n = list_length(in_count);
  DeviceScene S = A.scene;
  S.tex_counter = nullptr;
  for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
    const uint32_t i = base + threadIdx.x;
    guide_continue_ray<false>(A, S, i, i < n, may_push != 0u, hit, inst, in_o, in_d, out_o, out_d, out_count, aov0, aov1);
  }
}

struct ListSource {
  const float4* o;
  const float4* d;
  uint32_t n;
  __device__ __forceinline__ bool load(uint32_t i, vec3& origin, vec3& direction, float& tmin, float& tmax) {
    if (i >= n) return false;
    const float4 ro = o[i], rd = d[i];
    origin = mk3(ro.x, ro.y, ro.z);
    direction = mk3(rd.x, rd.y, rd.z);
    tmin = 0.0001f;   // as CentreSource
    tmax = INFINITY;
    return true;
  }
};
__global__ void __launch_bounds__(kBlock) k_guide_trace(const LaunchArgs A, const float4* __restrict__ in_o, const float4* __restrict__ in_d, const uint32_t* in_count,
                                                        float4* hit, uint32_t* inst) {
  __shared__ int s_stack[kLdsStack * kBlock];
  __shared__ alignas(1024) int s_aux[kAuxPerBlock];
  __shared__ uint4 s_top[kBvhTopNodes * 4];
  __shared__ float s_top_ray[9 * kBlock];
  const uint32_t n = list_length(in_count);
  if (n == 0) return;   // (the whole grid: nothing has been staged, no barrier is waiting)
  stage_top(A.scene, s_top);
  TraceTally tally;
  ListSource src{in_o, in_d, n};
  HitSink<false> sink{A, hit, inst};
  if (A.scene.two_level) trace_wave_tl<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), &s_top_ray[threadIdx.x], (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
  else trace_wave<false, false>(A.scene, src, sink, &s_stack[threadIdx.x], wave_aux(s_aux, threadIdx.x >> 6), wave_links(s_aux, threadIdx.x >> 6), (LdsNodePtr)s_top, A.st.overflow, A.st.overflow_depth, n, wave_index(), wave_count(), tally);
}
// a list back to the pixels it belongs to (glz_debug_guide_chain): 3 floats each, row-major, and alive = 1; the rest is left as it is
__global__ void __launch_bounds__(kBlock) k_guide_scatter(const float4* __restrict__ in_o, const float4* __restrict__ in_d, const uint32_t* in_count, uint32_t n_pixels,
                                                          float* __restrict__ o3, float* __restrict__ d3, uint8_t* __restrict__ alive) {
  const uint32_t n = list_length(in_count);
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const float4 ro = in_o[i], rd = in_d[i];
    const uint32_t p = __float_as_uint(rd.w);
    if (p >= n_pixels) continue;
    o3[3 * (size_t)p] = ro.x; o3[3 * (size_t)p + 1] = ro.y; o3[3 * (size_t)p + 2] = ro.z;
    d3[3 * (size_t)p] = rd.x; d3[3 * (size_t)p + 1] = rd.y; d3[3 * (size_t)p + 2] = rd.z;
    alive[p] = 1;
  }
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
// Firefly rejection (glz_despeckle_params; post::despeckle_pixel holds the arithmetic).  k_atrous's layout: every window row a wave reads is
// one coalesced line per plane (the colours as 16-byte lanes, the depths as the .w dwords of theirs), requested together before the first
// value is used; columns outside the image read the clamped column and are dropped.  The window's L values stay in registers (RADIUS is a
// template parameter: both loops unroll), M comes from a sorted top-4 kept by compare and select: no loop with a data-dependent trip count,
// no LDS, no scratch.  Two correctly rounded divisions per pixel that is clamped, one per candidate that is not.
// REMODULATE: out = i_0' * max(albedo, eps_a), the stand-alone read; otherwise out = i_0', what the filter's first pass reads.
// ---------------------------------------------------------------------------------------------
template <int RADIUS, bool REMODULATE>
__global__ void __launch_bounds__(kBlock) k_despeckle(uint32_t w, uint32_t h, uint32_t trim, float ratio, float eps_albedo, const float4* __restrict__ in,
                                                      const float4* __restrict__ aov0, const float4* __restrict__ aov1, float4* __restrict__ out) {
  const uint32_t x = blockIdx.x * kPostTileW + (threadIdx.x & 63u), y = blockIdx.y * kPostTileH + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  float4 v = post::despeckle_pixel<RADIUS>(in, aov0, w, h, x, y, trim, ratio);
  const size_t p = (size_t)y * w + x;
  if (REMODULATE) v = post::remodulate(v, aov1[p], eps_albedo);
  out[p] = v;
}

// ---------------------------------------------------------------------------------------------
// Motion and reprojection (glz_renderer_read_motion, glz_renderer_reproject; post::project_point and post::reproject_pixel hold the
// arithmetic, shared with the host references).
//   k_motion     one thread per pixel (row-major), after k_first_hit and before anything reuses the hit buffers: the hit record and the
//                instance, the three position float4s and the transform word of the shading record (rec[0], rec[2], rec[4], rec[7]: one
//                128-byte line), 64 B of the previous object -> world matrix (the caller's, 64 B apart, or the scene's own, the first half
//                of its 128-byte TransformPair), one float4 out.  Record, point and transform index are hit_vertex.h's; nothing is skipped
//                for a transform flagged identity: the previous one need not be.
//   k_motion_deform  k_motion for meshes that deformed (glz_previous_state::vertices): the object-space point comes from the PREVIOUS
//                positions of the hit triangle's vertices, which no record holds, so the kernel walks to them: the hit record and the
//                instance, then the leaf's primitive number (4 B of its BvhTri) and the RTInstance (16 B) together, then the three indices
//                and the 64 B of the previous matrix together, then three position float4s -- from the caller's array for an index inside
//                [first, first + count), from the scene's own vertices otherwise: the base pointer is selected, the load is one and
//                unconditional.  Four dependent levels, nothing in a level waits for another of the same level; the shading record is not
//                read.  Instance and transform are what k_motion takes: a flat scene's record carries the transform id of the leaf's instance.
//                Both kernels are motion_pixel, so the arithmetic behind the point is one text.  No LDS, no scratch, no loop.
//   k_reproject  k_atrous's layout.  A wave's taps sit at p + motion with nearly equal motion, so they fall in a few lines; every load is
//                requested before the first is used.  No LDS, no scratch, no loop with a data-dependent trip count.
// ---------------------------------------------------------------------------------------------
struct PrevVertices {
  const float4* v;         // device: the caller's glz_vertex array as it is, two float4 per vertex, the position in the first
  uint32_t first, count;   // the scene's vertices [first, first + count)
};
template <bool DEFORM>
__device__ __forceinline__ void motion_pixel(const DeviceScene& S, uint32_t w, uint32_t h, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                             const float4* __restrict__ prev_o2w, const PrevVertices& V, const post::ProjectConstants& C, float4* __restrict__ out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= w * h) return;
  const float4 hr = hit[p];
  uint32_t hit_inst = 0;
  if (DEFORM) {   // requested beside the record, not behind the miss test: the walk starts from both (a miss's is read and dropped)
    hit_inst = inst[p];
    asm volatile("" : "+v"(hit_inst));   // (no instruction: it keeps the compiler from sinking the load behind the branch, where it would wait alone)
  }
  const uint32_t leaf = __float_as_uint(hr.w);
  if (leaf == 0xFFFFFFFFu) {
    out[p] = make_float4(0.0f, 0.0f, INFINITY, __uint_as_float(0xFFFFFFFFu));
    return;
  }
  if (!DEFORM) hit_inst = inst[p];
  uint32_t xf;
  vec3 point;
  float4 m0, m1, m2, m3;
  if (DEFORM) {
    const uint32_t prim = S.bvh_tris[leaf].prim_flags & kTriPrimMask;
    const RTInstance in = S.instances[hit_inst];   // flat: the leaf's own instance; two levels: the leaf is the mesh's, whose indices the instance names
    const uint32_t* ix = S.indices + in.index_offset + 3u * (size_t)prim;
    const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
    xf = in.transform_id;
    const float4* xq = prev_o2w ? prev_o2w + 4u * (size_t)xf : reinterpret_cast<const float4*>(&S.transforms[xf]);
    m0 = xq[0], m1 = xq[1], m2 = xq[2], m3 = xq[3];
    const auto position = [&](uint32_t i) {   // (i - first wraps for i < first: not below count)
      const bool previous = i - V.first < V.count;
      return (previous ? V.v : S.vertices)[2u * (size_t)(previous ? i - V.first : i)];
    };
    const float4 a = position(i0), b = position(i1), c = position(i2);
    point = hit_point(a, b, c, hr);
  } else {
    const ShadeRecord rec = load_shade_record(S, leaf);
    xf = hit_ids<false>(S, rec, [&]() { return hit_inst; }).xf;
    point = hit_point(rec, hr);
    const float4* xq = prev_o2w ? prev_o2w + 4u * (size_t)xf : reinterpret_cast<const float4*>(&S.transforms[xf]);
    m0 = xq[0], m1 = xq[1], m2 = xq[2], m3 = xq[3];
  }
  const float o2w[16] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z, m3.w};
  const vec3 prev = xform_point(o2w, point);
  out[p] = post::motion_value(C, w, h, p % w, p / w, prev.x, prev.y, prev.z, __uint_as_float(hit_inst));
}
__global__ void __launch_bounds__(kBlock) k_motion(const DeviceScene S, uint32_t w, uint32_t h, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                                   const float4* __restrict__ prev_o2w, const post::ProjectConstants C, float4* __restrict__ out) {
  motion_pixel<false>(S, w, h, hit, inst, prev_o2w, PrevVertices{nullptr, 0u, 0u}, C, out);
}
__global__ void __launch_bounds__(kBlock) k_motion_deform(const DeviceScene S, uint32_t w, uint32_t h, const float4* __restrict__ hit, const uint32_t* __restrict__ inst,
                                                          const float4* __restrict__ prev_o2w, const PrevVertices V, const post::ProjectConstants C,
                                                          float4* __restrict__ out) {
  motion_pixel<true>(S, w, h, hit, inst, prev_o2w, V, C, out);
}
__global__ void __launch_bounds__(kBlock) k_reproject(uint32_t w, uint32_t h, float tolerance, const float4* __restrict__ motion, const float4* __restrict__ color,
                                                      const float4* __restrict__ aov0, const float4* __restrict__ aov1, float4* __restrict__ out) {
  const uint32_t x = blockIdx.x * kPostTileW + (threadIdx.x & 63u), y = blockIdx.y * kPostTileH + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  out[(size_t)y * w + x] = post::reproject_pixel(motion, color, aov0, aov1, w, h, x, y, tolerance);
}
// post::project_point of n points (3 floats each): the parity hook behind glz_debug_project_points
__global__ void __launch_bounds__(kBlock) k_project_points(const post::ProjectConstants C, float w, float h, const float* __restrict__ points3, uint32_t n,
                                                           float* __restrict__ out3) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const post::Projected r = post::project_point(C, w, h, points3[3 * (size_t)i], points3[3 * (size_t)i + 1], points3[3 * (size_t)i + 2]);
  out3[3 * (size_t)i] = r.fx; out3[3 * (size_t)i + 1] = r.fy; out3[3 * (size_t)i + 2] = r.z;
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
  return launch_per_item(st, k_first_hit_attributes, a.map.width * a.map.height, a, hit, inst, aov0, aov1);
}
// blocks of k_guide_trace's persistent grid: the tracers' residency rule, and never more than the first-hit pass's, whose spill area it uses
uint32_t guide_grid_blocks(uint32_t n_rays, uint32_t first_hit_blocks) { return std::min(persistent_grid(k_guide_trace, n_rays).x, first_hit_blocks); }
hipError_t launch_guide_chain(hipStream_t st, const LaunchArgs& a, uint32_t blocks, uint32_t max_bounces, uint32_t last_list, float4* hit, uint32_t* inst,
                              const GuideLists& lists, float4* aov0, float4* aov1) {
  const uint32_t n = a.map.width * a.map.height;
  if (n == 0) return hipSuccess;
  if (a.map.rank != 0 || a.map.world != 1 || max_bounces < 1 || max_bounces > GLZ_GUIDE_MAX_BOUNCES || last_list < 1) return hipErrorInvalidValue;
  if (blocks == 0 || (uint64_t)blocks * kBlock > (uint64_t)a.map.n_local_pixels + kBlock) return hipErrorInvalidValue;   // the spill area, as launch_first_hit
  hipError_t status = hipMemsetAsync(lists.count, 0, sizeof(uint32_t) * kGuideCountWords, st);
  if (status != hipSuccess) return status;
  hipLaunchKernelGGL(k_guide_first, grid_for(n), dim3(kBlock), 0, st, a, hit, inst, lists.o[1], lists.d[1], lists.count + 1, aov0, aov1);
  for (uint32_t k = 1; k <= max_bounces && k < last_list; ++k) {   // list k -> hits -> vertex k -> list k + 1 (none behind vertex max_bounces)
    const uint32_t in = k & 1u, out = in ^ 1u;
    hipLaunchKernelGGL(k_guide_trace, dim3(blocks), dim3(kBlock), 0, st, a, lists.o[in], lists.d[in], lists.count + k, hit, inst);
    hipLaunchKernelGGL(k_guide_continue, dim3(blocks), dim3(kBlock), 0, st, a, k < max_bounces ? 1u : 0u, hit, inst, lists.o[in], lists.d[in], lists.count + k, lists.o[out],
                       lists.d[out], lists.count + k + 1, aov0, aov1);
  }
  return hipGetLastError();
}
hipError_t launch_guide_scatter(hipStream_t st, uint32_t blocks, const GuideLists& lists, uint32_t list, uint32_t n_pixels, float* origins3, float* dirs3, uint8_t* alive) {
  if (n_pixels == 0) return hipSuccess;
  if (blocks == 0 || list < 1 || list > GLZ_GUIDE_MAX_BOUNCES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_guide_scatter, dim3(blocks), dim3(kBlock), 0, st, lists.o[list & 1u], lists.d[list & 1u], lists.count + list, n_pixels, origins3, dirs3, alive);
  return hipGetLastError();
}
hipError_t launch_camera_rays(hipStream_t st, const LaunchArgs& a, float off_x, float off_y, float* origins3, float* dirs3) {
  return launch_per_item(st, k_camera_rays, a.map.width * a.map.height, a, off_x, off_y, origins3, dirs3);
}
static dim3 post_tile_grid(uint32_t w, uint32_t h) { return dim3((w + kPostTileW - 1) / kPostTileW, (h + kPostTileH - 1) / kPostTileH); }
template <bool REMODULATE>
static void launch_despeckle_kernel(hipStream_t st, uint32_t w, uint32_t h, const glz_despeckle_params& D, float eps_albedo, const float4* in, const float4* aov0,
                                    const float4* aov1, float4* out, hipEvent_t* marks) {
  if (marks) (void)hipEventRecord(marks[0], st);
  if (D.radius == 1u) hipLaunchKernelGGL((k_despeckle<1, REMODULATE>), post_tile_grid(w, h), dim3(kBlock), 0, st, w, h, D.trim, D.ratio, eps_albedo, in, aov0, aov1, out);
  else hipLaunchKernelGGL((k_despeckle<2, REMODULATE>), post_tile_grid(w, h), dim3(kBlock), 0, st, w, h, D.trim, D.ratio, eps_albedo, in, aov0, aov1, out);
  if (marks) (void)hipEventRecord(marks[1], st);
}
hipError_t launch_denoise(hipStream_t st, uint32_t w, uint32_t h, const glz_denoise_params& P, const float4* result, const float4* aov0, const float4* aov1,
                          float4* ping, float4* pong, float4* out, hipEvent_t* marks, const glz_despeckle_params* despeckle, hipEvent_t* despeckle_marks) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!post::denoise_params_valid(P) || (uint64_t)w * h > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (despeckle && !post::despeckle_params_valid(*despeckle)) return hipErrorInvalidValue;
  const uint32_t n = w * h;
  if (marks) (void)hipEventRecord(marks[0], st);
  hipLaunchKernelGGL(k_demodulate, grid_for(n), dim3(kBlock), 0, st, n, result, aov1, P.eps_albedo, ping);
  if (marks) (void)hipEventRecord(marks[1], st);
  const float4* src = ping;
  if (despeckle) {   // ping -> pong, and the passes start from pong: no pixel sees a clamped neighbour, no further frame is needed
    launch_despeckle_kernel<false>(st, w, h, *despeckle, P.eps_albedo, ping, aov0, aov1, pong, despeckle_marks);
    src = pong;
  }
  const dim3 grid = post_tile_grid(w, h);
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
hipError_t launch_despeckle(hipStream_t st, uint32_t w, uint32_t h, const glz_despeckle_params& D, float eps_albedo, const float4* result, const float4* aov0,
                            const float4* aov1, float4* ping, float4* out, hipEvent_t* despeckle_marks) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!post::despeckle_params_valid(D) || (uint64_t)w * h > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint32_t n = w * h;
  hipLaunchKernelGGL(k_demodulate, grid_for(n), dim3(kBlock), 0, st, n, result, aov1, eps_albedo, ping);
  launch_despeckle_kernel<true>(st, w, h, D, eps_albedo, ping, aov0, aov1, out, despeckle_marks);
  return hipGetLastError();
}
hipError_t launch_motion(hipStream_t st, const LaunchArgs& a, const float4* hit, const uint32_t* inst, const float4* prev_o2w, const post::ProjectConstants& prev,
                         float4* motion, const float4* prev_vertices, uint32_t first_vertex, uint32_t n_vertices) {
  if (!prev_vertices) return launch_per_item(st, k_motion, a.map.width * a.map.height, a.scene, a.map.width, a.map.height, hit, inst, prev_o2w, prev, motion);
  if (n_vertices == 0) return hipErrorInvalidValue;
  return launch_per_item(st, k_motion_deform, a.map.width * a.map.height, a.scene, a.map.width, a.map.height, hit, inst, prev_o2w,
                         PrevVertices{prev_vertices, first_vertex, n_vertices}, prev, motion);
}
hipError_t launch_reproject(hipStream_t st, uint32_t w, uint32_t h, const glz_reproject_params& P, const float4* motion, const float4* prev_color,
                            const float4* prev_aov0, const float4* prev_aov1, float4* out, hipEvent_t* marks) {
  if (w == 0 || h == 0) return hipSuccess;
  if (!post::reproject_params_valid(P) || (uint64_t)w * h > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (marks) (void)hipEventRecord(marks[0], st);
  hipLaunchKernelGGL(k_reproject, post_tile_grid(w, h), dim3(kBlock), 0, st, w, h, P.depth_tolerance, motion, prev_color, prev_aov0, prev_aov1, out);
  if (marks) (void)hipEventRecord(marks[1], st);
  return hipGetLastError();
}
hipError_t launch_project_points(hipStream_t st, const post::ProjectConstants& C, uint32_t w, uint32_t h, const float* points3, uint32_t n, float* out3) {
  return launch_per_item(st, k_project_points, n, C, (float)w, (float)h, points3, n, out3);
}

}  // namespace glz
