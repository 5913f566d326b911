// hit_vertex: from a closest-hit record to the surface vertex (raytrace_hit.rchit:30-71) -- the one definition behind shade_pixel_body
// (k_shade, k_path), guide_vertex (the first-hit attributes and the guide chain) and k_motion (kernels_post.hip).  What one caller
// does not read the compiler drops: every step is forced inline and nothing here has a side effect.
#pragma once
#include "device/shading.h"

namespace glz {
using namespace dev;

struct ShadeRecord { float4 va0, va1, vb0, vb1, vc0, vc1, dn, du; };   // the 128-byte per-leaf shading record, as stored
struct HitVertex {
  ShadeRecord rec;     // (the texture level of detail works on the raw words)
  uint32_t xf_bits;    // transform index, bit 31: the transform is an exact identity
  vec3 point;
  vec2 uv;
  vec3 ng, ns, dpdu;   // dpdv is transformed by the reference but never read afterwards
  MatScalars mat;
};

__device__ __forceinline__ ShadeRecord load_shade_record(const DeviceScene& S, uint32_t leaf) {
  const float4* rec = S.shade_tris + 8u * (size_t)leaf;
  return ShadeRecord{rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]};
}
// the point of the hit `hr` = (t, u, v, leaf) on the triangle (a, b, c), the corners in index-buffer order (.w is not read)
__device__ __forceinline__ vec3 hit_point(float4 a, float4 b, float4 c, float4 hr) {
  const float b0 = 1.0f - hr.y - hr.z, b1 = hr.y, b2 = hr.z;
  return (mk3(a.x, a.y, a.z) * b0 + mk3(b.x, b.y, b.z) * b1) + mk3(c.x, c.y, c.z) * b2;
}
// the object-space point of the hit, from the record's positions
__device__ __forceinline__ vec3 hit_point(const ShadeRecord& r, float4 hr) { return hit_point(r.va0, r.vb0, r.vc0, hr); }
// Material and transform of the hit.  In two-level scenes the record is per OBJECT triangle and both are the instance's: `inst_of()`
// gives its index and is called in those scenes only.  FLAG: xf carries in bit 31 that the transform is an exact identity (a flat scene's
// record has the bit, S.xf_identity is read for an instance); without, xf is the plain index and nothing more is read.
struct HitIds { uint32_t material_id, xf; };
template <bool FLAG, class InstOf>
__device__ __forceinline__ HitIds hit_ids(const DeviceScene& S, const ShadeRecord& r, InstOf inst_of) {
  HitIds ids{__float_as_uint(r.dn.w), __float_as_uint(r.du.w)};
  if (!FLAG) ids.xf &= 0x7FFFFFFFu;
  if (S.two_level) {
    const RTInstance in = S.instances[inst_of()];
    ids.material_id = in.material_id;
    ids.xf = in.transform_id;
    if (FLAG) ids.xf = in.transform_id | (S.xf_identity[in.transform_id] ? 0x80000000u : 0u);
  }
  return ids;
}
// The vertex in OBJECT space, before the normal map: record, instance, barycentric point / uv / shading normal, material scalars.
template <class InstOf>
__device__ __forceinline__ HitVertex load_hit_vertex(const DeviceScene& S, float4 hr, InstOf inst_of) {
  HitVertex v;
  v.rec = load_shade_record(S, __float_as_uint(hr.w));
  const ShadeRecord& r = v.rec;
  const HitIds ids = hit_ids<true>(S, r, inst_of);
  const float b0 = 1.0f - hr.y - hr.z, b1 = hr.y, b2 = hr.z;
  v.point = hit_point(r, hr);
  v.uv = vec2{(r.va1.z * b0 + r.vb1.z * b1) + r.vc1.z * b2, (r.va1.w * b0 + r.vb1.w * b1) + r.vc1.w * b2};
  v.ng = mk3(r.dn.x, r.dn.y, r.dn.z), v.dpdu = mk3(r.du.x, r.du.y, r.du.z);
  v.ns = (mk3(r.va0.w, r.va1.x, r.va1.y) * b0 + mk3(r.vb0.w, r.vb1.x, r.vb1.y) * b1) + mk3(r.vc0.w, r.vc1.x, r.vc1.y) * b2;
  v.mat = load_material(S, ids.material_id);
  v.xf_bits = ids.xf;
  return v;
}
// The normal map at the footprint `fp`, then object -> world.  POINTS: `point` and `dpdu` are transformed too (a caller that goes on
// along the path needs them; the normals always are).  SHORT: the sampler's short forms (device/shading.h, texel_address); the post stage
// passes false and keeps the code it had.
template <bool POINTS, bool SHORT = true>
__device__ __forceinline__ void finish_hit_vertex(const DeviceScene& S, HitVertex& v, const TexFootprint& fp) {
  if (v.mat.normal != 0) {
    const vec4 tx = texture2d_lod<SHORT>(S, v.mat.normal, v.uv.x, v.uv.y, fp);
    Frame old;
    old.s = normalize3(v.dpdu);
    old.n = v.ns;
    old.t = normalize3(cross3(old.n, old.s));
    v.ns = normalize3(to_world(mk3(tx.x * 2.0f - 1.0f, tx.y * 2.0f - 1.0f, tx.z * 2.0f - 1.0f), old));
    v.ns = v.ns * gl_sign(dot3(v.ng, v.ns));
  }
  if (!(v.xf_bits >> 31)) {
    // Skipped for an exact identity transform: m*x with m = I reproduces x bit for bit
    // (x*1 + y*0 + z*0 + 0 for finite coordinates), so the result is unchanged and ~25 scalar loads are saved.
    const float4* xq = reinterpret_cast<const float4*>(&S.transforms[v.xf_bits & 0x7FFFFFFFu]);
    const float4 m0 = xq[0], m1 = xq[1], m2 = xq[2], m3 = xq[3], w0 = xq[4], w1 = xq[5], w2 = xq[6];
    const float w2o[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
    if (POINTS) {
      const float o2w[16] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w, m3.x, m3.y, m3.z, m3.w};
      v.point = xform_point(o2w, v.point);
      v.dpdu = xform_point(o2w, v.dpdu);   // transformed as a point, w = 1 (Q8)
    }
    v.ng = xform_tdir(w2o, v.ng);
    v.ns = xform_tdir(w2o, v.ns);
  }
}
// The surface point the BSDFs work on at the finished vertex, reached along `direction`: frame, material, the material's textures at `fp`.
template <bool SHORT = true>
__device__ __forceinline__ SurfacePoint hit_surface_point(const DeviceScene& S, const HitVertex& v, vec3 direction, const TexFootprint& fp) {
  SurfacePoint P;
  P.woW = -direction;
  P.uv = v.uv;
  P.frame = make_frame(v.dpdu, v.ns);
  P.mat = v.mat;
  fetch_material_textures<SHORT>(S, P, fp);
  return P;
}
}  // namespace glz
