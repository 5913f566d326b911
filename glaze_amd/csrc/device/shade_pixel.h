// shade_pixel: one pixel's shading step, shared by k_shade (kernels_render.hip) and k_path (kernels_path.hip), with the policies
// that say where its shadow-queue entry and its next path state go.
#pragma once
#include <hip/hip_runtime.h>

#include "device/hit_vertex.h"
#include "device/math.h"
#include "device/path_state.h"
#include "device/shading.h"
#include "device/types.h"
#include "kernels.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// One pixel of path_trace.rgen:170-237 minus the two traceRayEXT calls, with raytrace_hit.rchit:30-71 in front: what k_shade
// runs for the pixel at its sorted slot and what k_path (the per-wave launch loop of a small tile share) runs for each of a
// wave's 64 pixels.  `hr` is the closest-hit record of this launch, `queue.slot(push)` hands out the shadow-queue entry (all
// lanes that get this far call it together).
// ---------------------------------------------------------------------------------------------
struct SharedQueue {   // k_shade: the rank's sharded queue in HBM, drained by the next k_trace
  const LaunchArgs& A;
  __device__ __forceinline__ uint32_t slot(bool push) { return queue_slot(A.st.queue_count + A.shade_set * kQueueSetWords, A.map.n_local_pixels, push); }
};
// LOD: the build with the texture level of detail (FrameData::lod_mode != 0); the default build carries none of its code
// Where the pixel's next path state goes.  DirectState: straight into the state arrays (k_path: a wave's 64 pixels are neighbours, every
// store is whole lines).  StagedState (k_shade, whose threads shade pixels in regrouped order): kept in registers, the kernel writes
// them after the block's last barrier, transposed through LDS so that thread i stores pixel i's state.
// (k_shade: every thread storing its pixel's state itself 0.346 ms, the path state through the LDS transpose 0.322, the accumulator
// update through it too 0.329 -- so only the path state is staged.)
#ifdef GLZ_SECTION_TIMES   // tools/gpu_shade_sections.py: shader clocks between the stamps of shade_pixel, per wave (k_shade only)
#define GLZ_SHADE_STAMP(k) out.stamp(k)
#else
#define GLZ_SHADE_STAMP(k) do { } while (0)
#endif
__device__ __forceinline__ uint32_t pixel_rng(const FrameData& F, PixelId px) {
  return pcg(__float_as_uint((float)F.seed) ^ pcg(__float_as_uint((float)px.x) ^ pcg(__float_as_uint((float)px.y))));
}
__device__ __forceinline__ uint32_t light_pick(const FrameData& F, uint32_t& rng) {
  return (uint32_t)gl_min(rand01(rng) * (float)F.lights_no, (float)(F.lights_no - 1u));
}
struct DirectState {
  const LaunchArgs& A;
  static constexpr bool kDeferSkyTexel = false;   // (sample_light: k_path has no registers for the fetch code a second time)
  static constexpr bool kHandLambert = false;     // (nor for sixteen more between the evaluation and the sample)
  __device__ __forceinline__ void stamp(int) {}
  // the bracket table of S.sky_cdf (sample_cdf), where the cdf is: in memory, behind it
  __device__ __forceinline__ const uint16_t* sky_bracket(const DeviceScene& S) const {
    return reinterpret_cast<const uint16_t*>(S.sky_marginal + sky_bracket_offset(S.sky_header.marginal_cdf_count));
  }
  __device__ __forceinline__ void ray_o(uint32_t lid, float4 v) { A.st.ray_o[lid] = v; }
  __device__ __forceinline__ void ray_d(uint32_t lid, float4 v) { A.st.ray_d[lid] = v; }
  __device__ __forceinline__ void imp(int q, uint32_t lid, float4 v) { A.st.imp[q][lid] = v; }
  __device__ __forceinline__ float4 read_imp(int q, uint32_t lid) const { return A.st.imp[q][lid]; }
  __device__ __forceinline__ float4 reset_origin(uint32_t, float4 ro) const { return ro; }   // (the caller read the whole of ray_o, a line per wave)
  // the pixel's RNG at the start of the launch (path_trace.rgen:143, Q11) and the light pick of direct_light() (:84-117), made here
  __device__ __forceinline__ uint32_t seed_rng(const FrameData& F, PixelId px) const { return pixel_rng(F, px); }
  __device__ __forceinline__ uint32_t pick_light(const FrameData& F, uint32_t& rng) const { return light_pick(F, rng); }
  __device__ __forceinline__ void accumulate(uint32_t lid, vec3 c, bool add, bool update, float mark) { accumulate_shaded(A, lid, c, add && isfinite(c.x + c.y + c.z), update, mark); }
};
struct StagedState {
#ifdef GLZ_SECTION_TIMES
  unsigned long long sec[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sec_last = 0;
  __device__ __forceinline__ void stamp(int k) {
    const unsigned long long now = __builtin_amdgcn_s_memtime();   // (no wait: a section is charged what the wave waited for in it, not what it asked for)
    sec[k] += now - sec_last;
    sec_last = now;
  }
#else
  __device__ __forceinline__ void stamp(int) {}
#endif
  static constexpr bool kDeferSkyTexel = true;
  static constexpr bool kHandLambert = true;
  // the bracket table of the sky's marginal cdf, staged next to it in LDS; null where the cdf stays in memory (a sky too tall for LDS: the full search)
  const uint16_t* lds_sky_bracket = nullptr;
  __device__ __forceinline__ const uint16_t* sky_bracket(const DeviceScene&) const { return lds_sky_bracket; }
  float4 ro, rd, im[4];
  uint32_t mask = 0;   // 1: ro, 2: rd, 4: im
  __device__ __forceinline__ void ray_o(uint32_t, float4 v) { ro = v; mask |= 1u; }
  __device__ __forceinline__ void ray_d(uint32_t, float4 v) { rd = v; mask |= 2u; }
  __device__ __forceinline__ void imp(int q, uint32_t, float4 v) { im[q] = v; mask |= 4u; }
  const LaunchArgs* A = nullptr;   // the accumulator is updated where the pixel is shaded
  // The importance the pixel arrived with: k_shade's prologue reads the block's 4 x 4 KB in whole lines, in pixel order, into LDS, and the
  // (up to three) reads of shade_pixel come from there -- read where they are used, by threads in regrouped order, they were twelve
  // scattered 16-byte accesses per pixel on the vector-memory path, which is what bounds the kernel.
  LdsNodePtr lds_imp = nullptr;   // &s_imp[pixel's index in the block] (a pointer that keeps its address space: ds_read_b128); component q at [q * kShadeBlockPixels]
  static constexpr uint32_t kShadeBlockPixels = 256;
  __device__ __forceinline__ float4 read_imp(int q, uint32_t) const {
    const u32x4 v = lds_imp[q * kShadeBlockPixels];
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
  // The origin an ended path restarts from when the camera ray is not made here (no FrameData::pregen): the only reader of ray_o.xyz in
  // k_shade, so the only place that loads it -- the bounce, ray_o.w, reaches shade_pixel through LDS from the prologue's read in pixel order.
  __device__ __forceinline__ float4 reset_origin(uint32_t lid, float4) const { return A->st.ray_o[lid]; }
  // k_shade's prologue made both for the sort key (the hash of the seed: eight v_mul_lo_u32 with the pick) and left them in LDS for the
  // thread at the pixel's sorted slot: {the RNG state, the light index}.  The state is the one the draws of shade_pixel_body continue
  // from -- after the pick where the material takes one, the seed's hash where it does not -- so the sequence is DirectState's.
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(3))) u32x2* LdsPickPtr;
  LdsPickPtr lds_pick = nullptr;   // &s_pick[pixel's index in the block]
  __device__ __forceinline__ uint32_t seed_rng(const FrameData&, PixelId) const { return (*lds_pick).x; }
  __device__ __forceinline__ uint32_t pick_light(const FrameData&, uint32_t&) const { return (*lds_pick).y; }
  __device__ __forceinline__ void accumulate(uint32_t lid, vec3 cc, bool add, bool update, float mark) { accumulate_shaded(*A, lid, cc, add && isfinite(cc.x + cc.y + cc.z), update, mark); }
};
// Returns 0 when the pixel's next path state has been written (or, with the direct-light integrator, is not needed), 1 / 2 when the path
// has ENDED and its reset is left to shade_pixel below: 1 = only ray_o is to be written (a miss: ray_d keeps its flag), 2 = ray_o and
// ray_d, the latter with the flag `end_w`.
template <bool LOD, class Queue, class State>
__device__ __forceinline__ int shade_pixel_body(const LaunchArgs& A, const DeviceScene& S, const FrameData& F, uint32_t lid, PixelId px, float4 ro, float4 rd, float4 hr, Queue& queue,
                                                State& out, float& end_w) {
  const bool fresh = F.direct_only || ro.w == 0.0f;
  float bounce = F.direct_only ? 0.0f : ro.w;
  const vec3 direction = mk3(rd.x, rd.y, rd.z);
  // The path's importance (16 floats) is read where it is used -- the radiance of the light sample, the roulette, the final product --
  // instead of once up front: held through texture fetches, light sampling and the two BSDF calls it set the kernel's register peak.
  // The re-reads hit the lines the first read brought in.
  auto load_importance = [&]() {
    asm volatile("" ::: "memory");   // a fresh read every time: merged with an earlier one the values would stay in registers in between
    Spec imp;
    if (fresh) {
      imp = spec_set(1.0f);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = out.read_imp(q, lid);
        imp.w[4 * q] = v.x; imp.w[4 * q + 1] = v.y; imp.w[4 * q + 2] = v.z; imp.w[4 * q + 3] = v.w;
      }
    }
    return imp;
  };
  const uint32_t leaf = __float_as_uint(hr.w);
  if (leaf == 0xFFFFFFFFu) {
    // miss: optional sky radiance, path reset (path_trace.rgen:170-179)
    uint32_t flags = 0;
    vec3 c = mk3(0.0f, 0.0f, 0.0f);
    if ((bounce == 0.0f || rd.w == 1.0f) && S.sky.tex_id > 0) {
      const vec3 w = normalize3(xform_dir(S.sky.world2obj, direction));   // sky_radiance, :75-82
      const float phi = glz_atan2f(w.y, w.x), theta = glz_acosf(w.z);
      const vec3 texel = texture_rgb(S, S.sky.tex_id, vec2{phi * kInv2Pi, theta * kInvPi});
      c = spec_to_rgb(spec_mul(load_importance(), from_illuminant_color(texel)));
      flags = kFlagUpdate;
    }
    if (flags != 0) out.accumulate(lid, c, true, true, F.update_mark);   // (a miss behind a diffuse bounce only counts: nothing to write)
    end_w = rd.w;
    return F.direct_only ? 0 : 1;   // RESET_PATH
  }
  // ---- closest-hit shader (raytrace_hit.rchit:30-71), inputs from the 128-byte per-leaf shading record ----
  HitVertex hv = load_hit_vertex(S, hr, [&]() { return A.st.hit_inst[lid]; });
  const MatScalars mat = hv.mat;
  GLZ_SHADE_STAMP(0);   // hit record -> shading record -> material scalars
  // ---- texture level of detail by ray cones (build-defined, off by default: the reference's stages sample level 0) ----
  // The cone of a camera path starts cone_width0 wide and widens by cone_spread per unit of distance along the whole path;
  // at a hit the footprint on the surface is width / |cos|, and a texture of W x H texels over a triangle with texture-space
  // area A_uv and world area A_w is minified by sqrt(A_uv W H / A_w) texels per unit length:
  // level = 0.5 log2(A_uv / A_w * width^2 / cos^2) + 0.5 log2(W H)      (Akenine-Moeller et al., ray cones)
  // lod mode 2 (anisotropic): the footprint is cone_w across and cone_w / |cos| along the projection m of the ray direction onto the
  // surface; taps = ceil(min(1 / |cos|, 16)) probes along m, each at the level of a footprint cone_w / |cos| / taps wide; m written in
  // the triangle's edges (least squares: it lies in their plane) gives the footprint's long axis in texture space.
  TexFootprint fp{kNoLod, 0.0f, 0.0f, 1u};
  float cone_w = 0.0f;
  if constexpr (LOD) {
    const auto& [va0, va1, vb0, vb1, vc0, vc1, dn, du_rec] = hv.rec;   // the triangle in object space
    // (the argument's value behind an empty asm: the compiler otherwise merges the two reads into one load from a chosen address, an argument's or
    // the state array's, which is generic and makes the load FLAT)
    float cone_in = F.cone_width0;
    asm volatile("" : "+v"(cone_in));
    if (!fresh) cone_in = A.st.cone[lid];
    cone_w = cone_in + F.cone_spread * hr.x;
    vec3 e1 = mk3(vb0.x, vb0.y, vb0.z) - mk3(va0.x, va0.y, va0.z), e2 = mk3(vc0.x, vc0.y, vc0.z) - mk3(va0.x, va0.y, va0.z);
    vec3 n = mk3(dn.x, dn.y, dn.z);
    if (!(hv.xf_bits >> 31)) {
      const TransformPair* xf = &S.transforms[hv.xf_bits & 0x7FFFFFFFu];
      e1 = xform_dir(xf->o2w, e1);
      e2 = xform_dir(xf->o2w, e2);
      n = xform_tdir(xf->w2o, n);
    }
    const vec3 cr = cross3(e1, e2);
    const float area2 = sqrtf(dot3(cr, cr));
    const float uva2 = fabsf((vb1.z - va1.z) * (vc1.w - va1.w) - (vc1.z - va1.z) * (vb1.w - va1.w));
    const float nn = dot3(n, n), nd = dot3(n, direction);
    const float cosv = fabsf(nd) / sqrtf(nn);
    const float x = ((uva2 / area2) * (cone_w * cone_w)) / (cosv * cosv);
    if (x >= 1.17549435e-38f && x <= 3.4e38f) {
      fp.lod_base = 0.5f * glz_log2f(x);
      if (F.lod_mode == 2u) {
        float ratio = 1.0f / cosv;
        ratio = ratio < 16.0f ? ratio : 16.0f;
        const float taps = -glz_floorf(-ratio);   // ceil
        const vec3 m = direction - n * (nd / nn);
        const float mm = dot3(m, m);
        if (taps > 1.0f && mm > 0.0f) {
          const float g11 = dot3(e1, e1), g12 = dot3(e1, e2), g22 = dot3(e2, e2), r1 = dot3(m, e1), r2 = dot3(m, e2);
          const float det = g11 * g22 - g12 * g12;
          const float ca = (r1 * g22 - r2 * g12) / det, cb = (r2 * g11 - r1 * g12) / det;
          const float len = (cone_w / cosv) / sqrtf(mm);
          const float du = (ca * (vb1.z - va1.z) + cb * (vc1.z - va1.z)) * len;
          const float dv = (ca * (vb1.w - va1.w) + cb * (vc1.w - va1.w)) * len;
          if (fabsf(du) <= 3.4e38f && fabsf(dv) <= 3.4e38f) {
            fp.du = du;
            fp.dv = dv;
            fp.taps = (uint32_t)taps;
            fp.lod_base = fp.lod_base - glz_log2f(taps);
          }
        }
      }
    }
  }
  finish_hit_vertex<true>(S, hv, fp);
  const vec3 point = hv.point, ns = hv.ns;
  // ---- raygen continues (path_trace.rgen:180-237) ----
  uint32_t rng = out.seed_rng(F, px);   // :143, Q11
  const SurfacePoint P = hit_surface_point(S, hv, direction, fp);
  GLZ_SHADE_STAMP(1);   // normal map, transform, frame, the material's textures
  float spec_flag;
  // A Lambert hit's value is the same spectrum in the evaluation and in the sample, from_surface_color(tint / pi): where the evaluation
  // ran, State::kHandLambert hands what it made to bsdf_sample (alive across the radiance and the roulette only)
  Spec lambert_value = spec_set(0.0f);
  bool have_lambert = false;
  if (mat.is_specular == 0) {
    // direct_light(), :84-117
    const uint32_t li = out.pick_light(F, rng);
    vec3 xi;
    xi.x = rand01(rng); xi.y = rand01(rng); xi.z = rand01(rng);
    LightSample ls;
    ls.pdf = 0.0f;
    sample_light<State::kDeferSkyTexel>(S, li, point, xi, F.scene_radius, ls, out.sky_bracket(S));
    GLZ_SHADE_STAMP(2);   // light sample
    vec3 c = mk3(0.0f, 0.0f, 0.0f);
    uint32_t flags = kFlagUpdate;
    vec3 sh_dir = mk3(0.0f, 0.0f, 0.0f);
    float sh_tmax = 0.0f;
    if (ls.pdf > 0.0f) {
      const float xi_b = rand01(rng);
      Spec value = spec_set(0.0f);
      const float bpdf = bsdf_eval(S, P, ls.wiW, xi_b, value);
      if (State::kHandLambert && mat.bsdf_index == kBsdfLambert) {
        lambert_value = value;
        have_lambert = true;
      }
      if (bpdf > 0.0f) {
        // weight_light = (1 or 0) * |cos| / pdf; radiance = value*emission*weight*lights_no*importance
        const float w_vis = 1.0f * (fabsf(dot3(ls.wiW, ns)) / ls.pdf);
        const float nl = (float)F.lights_no;
        const Spec emission = light_emission<State::kDeferSkyTexel>(S, ls);
        const Spec importance = load_importance();
        Spec rad;
        GLZ_BINS {
          const float rl = value.w[i] * emission.w[i];
          rad.w[i] = ((rl * w_vis) * nl) * importance.w[i];
        }
        c = spec_to_rgb(rad);
        if (!isfinite(c.x + c.y + c.z)) c = mk3(0.0f, 0.0f, 0.0f);     // a NaN / Inf sample adds nothing, occluded or not
        flags |= kFlagShadow;
        sh_dir = ls.wiW;
        sh_tmax = ls.distance - 1e-3f;
      }
    }
    // (no light sample: the reference adds rgb(0 * lights_no * importance), zero or (non-finite importance) a NaN that adds nothing)
    // shadow-ray queue (consumed by the next launch's k_trace); pixels without a shadow ray are accumulated right here
    const bool push = (flags & kFlagShadow) != 0;
    GLZ_SHADE_STAMP(3);   // BSDF evaluation, radiance, importance read
    const uint32_t slot = queue.slot(push);
    if (push) {
      A.st.sh_o[slot] = make_float4(point.x, point.y, point.z, sh_tmax);
      A.st.sh_d[slot] = make_float4(sh_dir.x, sh_dir.y, sh_dir.z, __uint_as_float(lid));
      A.st.contrib[slot] = make_float4(c.x, c.y, c.z, __uint_as_float(flags));
    } else {
      out.accumulate(lid, c, false, true, F.update_mark);   // c is (+0, +0, +0) here: the pixel is marked, its sum neither read nor written (accumulate_shaded)
    }
    spec_flag = 0.0f;
  } else {
    spec_flag = 1.0f;   // a specular bounce only counts (update_count without update_result): nothing to write
  }
  if (F.direct_only) return 0;
  GLZ_SHADE_STAMP(4);   // queue entry / accumulator update
  // Russian roulette (:197-210)
  float rr_scale = 1.0f;   // importance * 1.0f is importance, bit for bit: the paths that skip the roulette multiply by it too
  if (bounce > (float)(F.pt_steps / 2u)) {
    // the luminance of the importance is made here, by the bounces that play: taken where the light-sampling block read the importance, on
    // both sides of its branch, every hit made it and only these read it (the importance is in LDS in k_shade: the second read is cheap)
    const float kill = gl_max(0.05f, 1.0f - spec_luminance(load_importance()));
    if (rand01(rng) < kill) {
      end_w = spec_flag;
      return 2;
    }
    rr_scale = 1.0f / (1.0f - kill);
  }
  vec3 xi;
  xi.x = rand01(rng); xi.y = rand01(rng); xi.z = rand01(rng);
  Spec value = spec_set(0.0f);
  vec3 wiW = mk3(0.0f, 0.0f, 0.0f);
  const float pdf = bsdf_sample(S, P, xi, value, wiW, &lambert_value, State::kHandLambert && have_lambert);   // :212-218
  if (pdf == 0.0f) {
    end_w = spec_flag;
    return 2;
  }
  float weight = fabsf(dot3(wiW, ns));
  weight /= pdf;
  const Spec importance = spec_scale(load_importance(), rr_scale);
#pragma unroll
  for (int q = 0; q < 4; ++q)
    out.imp(q, lid, make_float4(importance.w[4 * q] * (value.w[4 * q] * weight), importance.w[4 * q + 1] * (value.w[4 * q + 1] * weight),
                                importance.w[4 * q + 2] * (value.w[4 * q + 2] * weight), importance.w[4 * q + 3] * (value.w[4 * q + 3] * weight)));
  bounce = bounce < (float)F.pt_steps ? bounce + 1.0f : 0.0f;   // :230-237
  GLZ_SHADE_STAMP(5);   // roulette, BSDF sample, new importance
  if constexpr (LOD) A.st.cone[lid] = cone_w;
  if (F.pregen && bounce == 0.0f) {   // the path has reached its last step: the next launch starts a new one (only its flag survives)
    end_w = spec_flag;
    return 2;
  }
  out.ray_o(lid, make_float4(point.x, point.y, point.z, bounce));
  out.ray_d(lid, make_float4(wiW.x, wiW.y, wiW.z, spec_flag));
  return 0;
}
// shade_pixel_body, then the reset of a path that ended (RESET_PATH, path_trace.rgen:170-179 / :197-218): ray_o.w = 0 tells the next launch
// to start a new path at this pixel.  With FrameData::pregen the new path's camera ray is made right here, from the next launch's
// pixel offset (camera_ray: the operations ClosestSource::load would run in the next launch, bit for bit), and ray_o.w = -0.0 says so --
// k_shade's regrouping puts the pixels that missed into waves of their own, so the code runs with full waves where the traversal
// kernel's refill ran it with a quarter of the lanes.
template <bool LOD, class Queue, class State>
__device__ __forceinline__ void shade_pixel(const LaunchArgs& A, const DeviceScene& S, const FrameData& F, uint32_t lid, PixelId px, float4 ro, float4 rd, float4 hr, Queue& queue,
                                            State& out) {
  float end_w = 0.0f;
  const int ended = shade_pixel_body<LOD>(A, S, F, lid, px, ro, rd, hr, queue, out, end_w);
  if (ended != 0) {
    if (F.pregen) {
      vec3 co, cd;
      camera_ray(A, F, px, F.next_pixel_offset[0], F.next_pixel_offset[1], co, cd);
      out.ray_o(lid, make_float4(co.x, co.y, co.z, __uint_as_float(kPregenBounceBits)));
      out.ray_d(lid, make_float4(cd.x, cd.y, cd.z, end_w));
    } else {
      const float4 o = out.reset_origin(lid, ro);
      out.ray_o(lid, make_float4(o.x, o.y, o.z, 0.0f));
      if (ended == 2) out.ray_d(lid, make_float4(rd.x, rd.y, rd.z, end_w));
    }
  }
}

// The scene tables every hit walks through -- [MatCompact x n_materials | MetalSpectra x n_metal_spectra | RTLight x n_rt_lights |
// TexDesc x n_textures] -- as k_shade and k_path stage them in LDS when they fit.  The materials' metal spectra (128 of an RTMaterial's
// 208 bytes) are there once per distinct pair, not once per material.  The two capacities differ: k_shade's pool also holds the pixels' importance and the sky's
// marginal cdf, so its table area is the smaller; k_path takes its copy from dynamic LDS, which it asks for only when the tables fit,
// so a scene with small tables buys residency.
constexpr uint32_t kShadeLdsTableBytes = 8192;   // k_shade (about 90 materials of one metal; larger tables are read from memory)
constexpr uint32_t kPathTableBytes = 16384;      // k_path (about 190 materials)
static_assert(sizeof(MatCompact) % 16 == 0 && sizeof(MetalSpectra) % 16 == 0 && sizeof(RTLight) % 16 == 0 && sizeof(TexDesc) % 16 == 0, "the tables are copied in 16-byte pieces");
struct SceneTables {
  uint32_t qm, qs, ql, qt;   // the four tables' sizes in 16-byte pieces
  __host__ __device__ explicit SceneTables(const DeviceScene& s)
      : qm(s.n_materials * (uint32_t)(sizeof(MatCompact) / 16)), qs(s.n_metal_spectra * (uint32_t)(sizeof(MetalSpectra) / 16)), ql(s.n_rt_lights * (uint32_t)(sizeof(RTLight) / 16)), qt(s.n_textures * (uint32_t)(sizeof(TexDesc) / 16)) {}
  __host__ __device__ uint32_t bytes() const { return (qm + qs + ql + qt) * 16u; }
  // the cooperative copy by a block of `block` threads (the caller's barrier ends it) ...
  __device__ __forceinline__ void stage(const DeviceScene& s, uint4* dst, uint32_t block) const {
    const uint4* gm = reinterpret_cast<const uint4*>(s.mat_compact);
    const uint4* gs = reinterpret_cast<const uint4*>(s.metal_spectra);
    const uint4* gl = reinterpret_cast<const uint4*>(s.lights);
    const uint4* gt = reinterpret_cast<const uint4*>(s.tex_desc);
    const uint32_t es = qm + qs, el = es + ql;
    for (uint32_t i = threadIdx.x; i < el + qt; i += block) dst[i] = i < qm ? gm[i] : (i < es ? gs[i - qm] : (i < el ? gl[i - es] : gt[i - el]));
  }
  // ... and the four table pointers of S onto the copy
  __device__ __forceinline__ void use(DeviceScene& S, const uint4* copy) const {
    S.mat_compact = reinterpret_cast<const MatCompact*>(copy);
    S.metal_spectra = reinterpret_cast<const MetalSpectra*>(copy + qm);
    S.lights = reinterpret_cast<const RTLight*>(copy + qm + qs);
    S.tex_desc = reinterpret_cast<const TexDesc*>(copy + qm + qs + ql);
  }
};

// The kernel's arguments, re-read: behind the empty asm the compiler no longer knows that the pointer is the one it has been loading
// from, so what follows loads the arguments it needs where it needs them (scalar loads from the kernarg segment) instead of keeping
// every pointer of LaunchArgs in SGPRs from the top of the kernel -- there are more of them than SGPRs, the overflow goes to VGPR
// lanes (v_writelane / v_readlane) and takes registers from the shading code.
typedef const __attribute__((address_space(4))) char* KernargPtr;
__device__ __forceinline__ KernargPtr reread_kernarg() {
  KernargPtr p = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
}  // namespace glz
