// Ray / box and ray / triangle for the tracers (device/trace_wave.h, device/trace_wave_tl.h): the slab test on a quantised box, the
// watertight triangle test on a leaf record, the alpha test of a candidate, and the record a traversal hands to its sink.
#pragma once
#include <hip/hip_runtime.h>

#include "device/math.h"
#include "device/shading.h"
#include "device/types.h"

namespace glz {
using namespace dev;

// ---------------------------------------------------------------------------------------------
// Ray / box and ray / triangle.  The triangle test (ray_quad below) is watertight, accepts a candidate iff tmin < t < tmax and
// culls no face (acceleration.rs:335-345); it stands in for the driver's intersector ([ext]).  Ties on t are broken by the smaller
// world triangle id so that the result does not depend on traversal order.
// ---------------------------------------------------------------------------------------------
// Slab test on a quantised box.  It only prunes: boxes are padded by 1/16 cell when they are quantised, which covers the
// rounding of the plane distances (< 0.01 cell), so it never rejects a box whose triangle the exact test below accepts.  The ray
// is mapped into grid units once (ig = cell / d, the addend grid_addend); a node word holds lo | hi << 16 of one axis, and a per-ray
// byte permutation picks the plane the ray meets first and the other one -- no min / max per axis.  Both plane distances of an axis
// then come from one packed v_pk_fma_f32.  The tracers are VALU-issue bound, so instructions per node visit are what counts.  ig is
// kept finite (grid_inv_dir), so no plane distance is ever NaN: a ray parallel to a slab gets +-1e30-scale distances whose signs
// still say on which side of each plane the origin lies.
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct SlabSel { uint32_t x, y, z; };   // v_perm_b32 selectors per axis
// returns the sort key of the child: entry distance (a positive float, so its bits order like the value) with its ten lowest bits
// replaced by the child index in bits 8..9 (`k` = child << 8) -- nearer first, ties (to 2^-13 of the distance) by child index; 0xFFFFFFFF
// for a missed child or an unused slot.  Bits 8..9 because (key & 0x300) IS the byte offset of the child's link in the wave's link
// scratch ([child][lane], 256 bytes a child, the area 1 KB aligned): the address of a sorted link is one v_and_or_b32 (it was three
// instructions per link with the index in the low bits)
// (the slab test is symmetric in lo / hi, so an unused slot cannot be excluded through its box: its link says so)
// cgn / cgf: the addends of the near and the far plane.  The flattened tracer passes the same vector twice; the two-level tracer
// widens every box by the instance's slack (cg -+ pad * |ig|) at no extra instruction.
// Grid coordinates are 15 bits wide, so a byte permute turns one into a float without a conversion: the bytes {0, q_lo, q_hi, 0x47}
// are 0x47000000 | q << 8, the float 32768 + q (exponent 2^15, q in the mantissa's bits 22..8).  The 32768 is folded into the addend
// of the plane distance (grid_ray: cg - 32768 ig), the selector names which half of the node word -- the plane the ray meets first
// (lo for ig >= 0, hi for ig < 0) or the other one: kSlabSelLo / kSlabSelHi, one XOR apart.  Two permutes per axis instead of one
// permute and two v_cvt_f32_u32: 9 VALU instructions fewer per node visit (rounds 1-2 needed six live selectors for this and spilt).
constexpr uint32_t kKeyDistanceMask = 0xFFFFFC00u, kKeyChild = 0x100u, kKeyChildMask = 0x300u;   // sort key = distance bits | child << 8
constexpr uint32_t kSlabSelLo = 0x0305040Cu, kSlabSelHi = 0x0307060Cu, kSlabSelFlip = kSlabSelLo ^ kSlabSelHi, kSlabMagic = 0x47000000u;
__device__ __forceinline__ uint32_t slab_sel(float ig) { return ig < 0.0f ? kSlabSelHi : kSlabSelLo; }
// CHECK_LINK = false: an unused slot is excluded by its box alone -- lo = the grid's top, hi = 0 on every axis, and with the near /
// far plane picked by the ray's sign such a box has t_near > t_far on every axis whatever the ray (the planes are 32 767 cells the
// wrong way round; distances are never NaN) -- four compares fewer per node visit.  The two-level tracer widens boxes by a per-ray
// pad that may exceed that in extreme cases and keeps the check.
// ORDER: which child a sorted key sequence names first.  Any-hit rays (GLZ_ANY_FAR_FIRST, trace_wave) want the child entered LAST:
//   kKeysNearFirst  the key above; the caller sorts ascending.
//   kKeysFarFirst   every ray of the pass is an any-hit ray: the same key with bit 0 set, 0 for a miss, and the caller sorts DESCENDING --
//                   no instruction more than nearest first.  Bit 0 keeps the key of child 0 at t0 == 0 (tmin is the caller's in the debug
//                   kernels) apart from the miss marker; it lies below the child bits and no one reads it.
//   kKeysPerLane    rays of both kinds in one pass (k_path's MIXED pass): `flip` = kKeyDistanceMask in an any-hit lane, 0 in a closest-hit
//                   lane -- the distance bits complemented, so that the ascending sort puts the farthest first; one v_xor_b32 per child.
//                   The largest such key is 0xFFFFFC00 | k, never the miss marker.
constexpr int kKeysNearFirst = 0, kKeysFarFirst = 1, kKeysPerLane = 2;
template <int ORDER>
constexpr uint32_t kKeyMiss = ORDER == kKeysFarFirst ? 0u : 0xFFFFFFFFu;
template <bool CHECK_LINK = true, int ORDER = kKeysNearFirst>
__device__ __forceinline__ uint32_t box_key(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t link, uint32_t k, SlabSel sel, vec3 ig, vec3 cgn, vec3 cgf,
                                            float tmin, float tmax, uint32_t flip = 0u) {
  // v_perm_b32: bytes 0..3 of the selector index the second operand, 4..7 the first (the node word), 0x0C is a zero byte
  const float nx = __uint_as_float(__builtin_amdgcn_perm(wx, kSlabMagic, sel.x)), fx = __uint_as_float(__builtin_amdgcn_perm(wx, kSlabMagic, sel.x ^ kSlabSelFlip));
  const float ny = __uint_as_float(__builtin_amdgcn_perm(wy, kSlabMagic, sel.y)), fy = __uint_as_float(__builtin_amdgcn_perm(wy, kSlabMagic, sel.y ^ kSlabSelFlip));
  const float nz = __uint_as_float(__builtin_amdgcn_perm(wz, kSlabMagic, sel.z)), fz = __uint_as_float(__builtin_amdgcn_perm(wz, kSlabMagic, sel.z ^ kSlabSelFlip));
  const f32x2 tx = __builtin_elementwise_fma(f32x2{nx, fx}, f32x2{ig.x, ig.x}, f32x2{cgn.x, cgf.x});
  const f32x2 ty = __builtin_elementwise_fma(f32x2{ny, fy}, f32x2{ig.y, ig.y}, f32x2{cgn.y, cgf.y});
  const f32x2 tz = __builtin_elementwise_fma(f32x2{nz, fz}, f32x2{ig.z, ig.z}, f32x2{cgn.z, cgf.z});
  const float t0 = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, tmin));
  const float t1 = fminf(fminf(tx.y, ty.y), fminf(tz.y, tmax));
  const uint32_t bits = ORDER == kKeysPerLane ? __float_as_uint(t0) ^ flip : __float_as_uint(t0);
  return (t0 <= t1 && (!CHECK_LINK || link != (uint32_t)kBvhEmptyChild)) ? ((bits & kKeyDistanceMask) | k | (ORDER == kKeysFarFirst ? 1u : 0u)) : kKeyMiss<ORDER>;
}
// The same test for a child of an 8-wide node (types.h BvhNode8): the child index takes three bits of the key (8..10)
// FAR (a pass of any-hit rays): bit 0 set and 0 for a miss, as kKeysFarFirst above -- the caller picks the LARGEST key
constexpr uint32_t kKey8DistanceMask = 0xFFFFF800u, kKey8ChildMask = 0x700u;
template <bool FAR = false>
__device__ __forceinline__ uint32_t box_key8(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t k, SlabSel sel, vec3 ig, vec3 cg, float tmin, float tmax) {
  const float nx = __uint_as_float(__builtin_amdgcn_perm(wx, kSlabMagic, sel.x)), fx = __uint_as_float(__builtin_amdgcn_perm(wx, kSlabMagic, sel.x ^ kSlabSelFlip));
  const float ny = __uint_as_float(__builtin_amdgcn_perm(wy, kSlabMagic, sel.y)), fy = __uint_as_float(__builtin_amdgcn_perm(wy, kSlabMagic, sel.y ^ kSlabSelFlip));
  const float nz = __uint_as_float(__builtin_amdgcn_perm(wz, kSlabMagic, sel.z)), fz = __uint_as_float(__builtin_amdgcn_perm(wz, kSlabMagic, sel.z ^ kSlabSelFlip));
  const f32x2 tx = __builtin_elementwise_fma(f32x2{nx, fx}, f32x2{ig.x, ig.x}, f32x2{cg.x, cg.x});
  const f32x2 ty = __builtin_elementwise_fma(f32x2{ny, fy}, f32x2{ig.y, ig.y}, f32x2{cg.y, cg.y});
  const f32x2 tz = __builtin_elementwise_fma(f32x2{nz, fz}, f32x2{ig.z, ig.z}, f32x2{cg.z, cg.z});
  const float t0 = fmaxf(fmaxf(tx.x, ty.x), fmaxf(tz.x, tmin));
  const float t1 = fminf(fminf(tx.y, ty.y), fminf(tz.y, tmax));
  return t0 <= t1 ? ((__float_as_uint(t0) & kKey8DistanceMask) | k | (FAR ? 1u : 0u)) : (FAR ? 0u : 0xFFFFFFFFu);   // (an unused slot's box is inverted: no ray enters it)
}
// the addend of a plane distance: plane q (a float 32768 + q out of box_key) is crossed at t = (32768 + q) ig + grid_addend = q ig - og ig
__device__ __forceinline__ float grid_addend(float og, float ig) { return fmaf(-32768.0f, ig, -(og * ig)); }

// 1 / d clamped to +-1e30: zero (or denormal) direction components must not produce inf - inf in the fma above --
// a ray with a NaN plane distance on every axis would pass every box test and walk the whole tree.
__device__ __forceinline__ float grid_inv_dir(float d) {
  const float i = 1.0f / d;
  return fabsf(i) <= 1e30f ? i : copysignf(1e30f, i);
}
// The same from the hardware's reciprocal (v_rcp_f32, one ulp) instead of the correctly rounded division (ten instructions): for the
// flattened tracer's refill, which runs with a quarter of the wave's lanes.  The grid-space ray only PRUNES -- hits come from the exact
// test on the world ray -- and an error of 2^-23 in ig moves a plane crossing by at most 32 768 cells x 2^-23 = 0.004 cell, inside the
// 1/16 cell the boxes are padded by (the rounding of the plane distances themselves takes 0.01).  The counting kernels keep the
// division: their node counts are compared with the oracle's walk.
__device__ __forceinline__ float grid_inv_dir_fast(float d) {
  const float i = __builtin_amdgcn_rcpf(d);
  return fabsf(i) <= 1e30f ? i : copysignf(1e30f, i);
}
// rays with a NaN / infinite origin or direction cannot be accepted by ray_quad (every comparison fails): they
// are reported as misses without traversal
__device__ __forceinline__ bool ray_is_finite(vec3 o, vec3 d) {
  const float s = ((o.x + o.y) + o.z) + ((d.x + d.y) + d.z);
  return s - s == 0.0f;
}

// The watertight ray / triangle test, statement for statement the oracle's ray_tri (oracle.cpp; the reference's hits come from
// traceRayEXT on the driver's acceleration structure, path_trace.rgen:169 / acceleration.rs:319-345, which the Vulkan
// specification requires to be watertight): Woop, Benthin, Wald 2013 with the exact tie-break in single precision.
//   per ray    kz = axis of the largest |d|, shear Sz = 1 / d[kz], Sx = d[kx] Sz, Sy = d[ky] Sz        (ray_shear; once per leaf round,
//              from d alone -- nothing is kept per ray, the traversal has no register to spare)
//   per vertex A = P - o, image (A[kx] - Sx A[kz], A[ky] - Sy A[kz], Sz A[kz]): the same 2-D point in every triangle that uses P
//   per edge   U = Cx By - Cy Bx from two separately rounded products: its sign is exact unless the rounded products are equal, and
//              then the difference of their rounding errors (one fma each) is.  Exact orientation predicates on consistent points
//              cannot leave a gap at a shared edge or vertex.  -ffp-contract=off keeps the products unfused.
// Straight-line: with ~10 of 64 lanes in a leaf round an early exit is almost never taken by all of them, and without branches
// the three 16-byte loads of the triangle are issued together; only the tie-break is a (wave-uniform) branch, taken when some
// lane's ray meets an edge exactly -- axis-aligned geometry under an orthographic camera, otherwise hardly ever.
struct RayShear {
  bool z_is_x, z_is_y;   // kz == 0, kz == 1 (else 2): wave masks in SGPRs
  float sx, sy, sz;
};
__device__ __forceinline__ RayShear ray_shear(vec3 d) {
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  RayShear r;
  r.z_is_x = (ax >= ay) & (ax >= az);
  r.z_is_y = !r.z_is_x & (ay >= az);
  // (kx, ky, kz) = (1, 2, 0), (2, 0, 1) or (0, 1, 2)
  const float dz = r.z_is_x ? d.x : (r.z_is_y ? d.y : d.z), dx = r.z_is_x ? d.y : (r.z_is_y ? d.z : d.x), dy = r.z_is_x ? d.z : (r.z_is_y ? d.x : d.y);
  r.sz = 1.0f / dz;
  r.sx = dx * r.sz;
  r.sy = dy * r.sz;
  return r;
}
constexpr float kDetNoise = 1.9073486e-6f;   // 2^-19 of three of the six products (about 2^-20 of their sum): see triangle_finish

// The test on a leaf record of the flattened build (types.h BvhQuad): triangle A = (q0, q1, q2) and, for a leaf of two,
// B = (q0, q2, q3).  Per triangle the operations and their order are the oracle's ray_tri on one 48-byte record (types.h BvhTri), so (t, u, v) and the verdict are bit for bit
// what the 48-byte records give; what the record saves is work the two triangles share: four vertex images instead of six, and the
// two products of the edge q0-q2 -- B's edge function along it is A's with the operands of the subtraction exchanged (the products
// themselves commute), tie-break terms included.  Straight-line: the four 16-byte loads of a leaf issue together.
struct QuadHit {
  float t[2], u[2], v[2];   // [0] = A, [1] = B
  bool ok[2];
};
__device__ __forceinline__ vec3 shear_point(const RayShear& r, float px, float py, float pz, vec3 o) {
  const vec3 a = mk3(px, py, pz) - o;
  const float az = r.z_is_x ? a.x : (r.z_is_y ? a.y : a.z), ax = r.z_is_x ? a.y : (r.z_is_y ? a.z : a.x), ay = r.z_is_x ? a.z : (r.z_is_y ? a.x : a.y);
  return mk3(fmaf(-r.sx, az, ax), fmaf(-r.sy, az, ay), r.sz * az);
}
// the part of a triangle's test behind the edge functions.  `products` = |first product of U| + |of V| + |of W|: a det smaller than kDetNoise
// of it is the products' rounding, not a number -- the ray lies in the triangle's plane as far as single precision can tell (a shadow
// ray towards a light in the plane of the surface it leaves), and the distance that would come out of it is anything.  The oracle's
// ray_tri has the same line; oracle.cpp says what it was found by.
__device__ __forceinline__ bool triangle_finish(float U, float V, float W, float Az, float Bz, float Cz, float products, float tmin, float& t, float& u, float& v) {
  const float lo = fminf(fminf(U, V), W), hi = fmaxf(fmaxf(U, V), W);
  const float det = (U + V) + W;
  const float inv = 1.0f / det;
  u = V * inv;
  v = W * inv;
  t = fmaf(W, Cz, fmaf(V, Bz, U * Az)) * inv;
  return !((lo < 0.0f) & (hi > 0.0f)) & (fabsf(det) > products * kDetNoise) & (t > tmin);
}
__device__ __forceinline__ QuadHit ray_quad(const RayShear& rs, float4 r0, float4 r1, float4 r2, float4 r3, bool pair, vec3 o, float tmin) {
  QuadHit h;
  const vec3 S0 = shear_point(rs, r0.x, r0.y, r0.z, o), S2 = shear_point(rs, r2.x, r2.y, r2.z, o);
  const float pv = S0.x * S2.y, qv = S0.y * S2.x;   // the shared edge q0-q2: V of A, W of B
  {
    // A = (S0, S1, S2):  U = C x B, V = A x C, W = B x A  with  A = S0, B = S1, C = S2
    const vec3 S1 = shear_point(rs, r1.x, r1.y, r1.z, o);
    const float pu = S2.x * S1.y, qu = S2.y * S1.x, pw = S1.x * S0.y, qw = S1.y * S0.x;
    float U = pu - qu, V = pv - qv, W = pw - qw;
    if (__builtin_expect(__any((U == 0.0f) | (V == 0.0f) | (W == 0.0f)), 0)) {   // edge_fn's second branch, for the lanes that need it
      if (U == 0.0f) U = fmaf(S2.x, S1.y, -pu) - fmaf(S2.y, S1.x, -qu);
      if (V == 0.0f) V = fmaf(S0.x, S2.y, -pv) - fmaf(S0.y, S2.x, -qv);
      if (W == 0.0f) W = fmaf(S1.x, S0.y, -pw) - fmaf(S1.y, S0.x, -qw);
    }
    h.ok[0] = triangle_finish(U, V, W, S0.z, S1.z, S2.z, (fabsf(pu) + fabsf(pv)) + fabsf(pw), tmin, h.t[0], h.u[0], h.v[0]);
  }
  __builtin_amdgcn_sched_barrier(0);   // A is finished before B begins: interleaved for ILP the two keep twice the values alive (20 registers spilt)
  {
    // B = (S0, S2, S3):  U = S3 x S2, V = S0 x S3, W = S2 x S0 = S2.x S0.y - S2.y S0.x = qv - pv
    const vec3 S3 = shear_point(rs, r3.x, r3.y, r3.z, o);
    const float pu = S3.x * S2.y, qu = S3.y * S2.x, pv2 = S0.x * S3.y, qv2 = S0.y * S3.x;
    float U = pu - qu, V = pv2 - qv2, W = qv - pv;
    if (__builtin_expect(__any(pair & ((U == 0.0f) | (V == 0.0f) | (W == 0.0f))), 0)) {
      if (U == 0.0f) U = fmaf(S3.x, S2.y, -pu) - fmaf(S3.y, S2.x, -qu);
      if (V == 0.0f) V = fmaf(S0.x, S3.y, -pv2) - fmaf(S0.y, S3.x, -qv2);
      if (W == 0.0f) W = fmaf(S2.x, S0.y, -qv) - fmaf(S2.y, S0.x, -pv);
    }
    h.ok[1] = triangle_finish(U, V, W, S0.z, S2.z, S3.z, (fabsf(pu) + fabsf(pv2)) + fabsf(qv), tmin, h.t[1], h.u[1], h.v[1]) & pair;
  }
  return h;
}

// raytrace_hit.rahit:24-39 -- candidates on non-opaque geometry are dropped when opacity.r < 0.5
__device__ __forceinline__ bool alpha_test(const DeviceScene& S, uint32_t leaf, float u, float v) {
  // One 48-byte record per triangle slot (types.h DeviceScene::alpha_recs; every flattened scene with an opacity map has them): the
  // three texture coordinates -- the values the reference's any-hit shader reads through instance -> indices -> vertices -- and the
  // descriptor of the material's opacity map: record -> texels, two round trips where shading record -> material -> descriptor ->
  // texels were four (a wave sits through them with the dozen lanes of an alpha phase: 0.07 ms of the Sponza-like atrium's k_trace).
  const float w = 1.0f - u - v;
  const float4* rec = S.alpha_recs + 3u * (size_t)leaf;
  const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
  const float tu = (r0.x * w + r0.z * u) + r1.x * v, tv = (r0.y * w + r0.w * u) + r1.y * v;
  const TexDesc t{__float_as_uint(r1.z), __float_as_uint(r1.w), __float_as_uint(r2.x), __float_as_uint(r2.y)};
  return !(bilinear_level<false>(S, t, S.tex_pool, tu, tv).x < 0.5f);   // (<false>: device/shading.h, texel_address)
}

// the same for a two-level scene: the shading record is per OBJECT triangle, the material is the instance's
__device__ __forceinline__ bool alpha_test_instance(const DeviceScene& S, uint32_t slot, uint32_t instance, float u, float v) {
  const float4* rec = S.shade_tris + 8u * (size_t)slot;
  const float4 a = rec[1], b = rec[3], c = rec[5];
  const uint32_t material_id = S.instances[instance].material_id;
  const float w = 1.0f - u - v;
  const float tu = (a.z * w + b.z * u) + c.z * v, tv = (a.w * w + b.w * u) + c.w * v;
  return !(texture_r<false>(S, S.materials[material_id].opacity, vec2{tu, tv}) < 0.5f);
}

struct HitRecord {
  float t, u, v;
  uint32_t leaf;   // index into bvh_tris / shade_tris, 0xFFFFFFFF = miss
  // two-level scenes only (a flattened triangle record names its instance itself):
  uint32_t inst;       // RTInstance of the hit
  uint32_t world_id;   // world triangle id (instance-major), the tie-break key
};
}  // namespace glz
