// Linear-blend skinning (glz_renderer_pose_skins, glz_host_skin; include/glaze_abi.h holds the specification): one vertex under four
// weighted bones, in the ONE form both the host reference (skin_host.cpp; g++) and the device kernel (kernels_skin.hip; hipcc) compile:
// the same operations in the same order, -ffp-contract=off on both sides, so the two agree bit for bit.  Only + and *, float32.
//
// The normal goes through the blended matrix's 3 x 3 as it is -- not through its inverse transpose, and it is not renormalised (shading
// normalises the normal it interpolates).  That is EXACT ONLY FOR RIGID BONES (rotation + translation) blended with weights that sum to 1;
// under scale, shear or other weights the normal is the blended matrix's image of the bind normal, no more.
//
// Dual-quaternion blending (GLZ_SKIN_DUAL_QUATERNION; "THE DUAL-QUATERNION RULE" in include/glaze_abi.h) is the second rule of this file,
// a per-skin mode next to the linear one and held to the same discipline: one definition for host and device, float32, + - *, one sqrtf
// and one 1.0f / x, both correctly rounded on either side (normals.h normalises the same way).  The blend of unit dual quaternions,
// normalised, IS a rigid motion, so the normal it gives is exact wherever the bones are rigid, whatever the weights.
#pragma once
#include <math.h>

#include "denoise.h"

namespace glz {
namespace post {

// A bone as the kernel reads it: the upper 3 x 4 of the column-major glz_transform as three rows of four, 48 bytes; row r = (m[r], m[4 + r],
// m[8 + r], m[12 + r]).  The transform's fourth row is not kept.
constexpr uint32_t kSkinBoneRows = 3;
inline void pack_bone(const glz_transform& b, float4 rows[kSkinBoneRows]) {
  for (uint32_t r = 0; r < kSkinBoneRows; ++r) rows[r] = make_float4(b.m[r], b.m[4 + r], b.m[8 + r], b.m[12 + r]);
}

// ((w0 * b0 + w1 * b1) + w2 * b2) + w3 * b3 per component: no term is skipped for a zero weight
GLZ_POST_FN float4 blend_row(float4 w, float4 b0, float4 b1, float4 b2, float4 b3) {
  return make_float4(((w.x * b0.x + w.y * b1.x) + w.z * b2.x) + w.w * b3.x, ((w.x * b0.y + w.y * b1.y) + w.z * b2.y) + w.w * b3.y,
                     ((w.x * b0.z + w.y * b1.z) + w.z * b2.z) + w.w * b3.z, ((w.x * b0.w + w.y * b1.w) + w.z * b2.w) + w.w * b3.w);
}

// One vertex: v0 = (p.xyz, n.x), v1 = (n.yz, t.uv) as the vertex buffer stores it, in and out; j: the four joints, each below the bone
// count (the caller has checked); w: the four weights, used as given; bones: kSkinBoneRows float4 per bone, in whichever memory Rows names.
template <class Rows>
GLZ_POST_FN void skin_vertex(Rows bones, const uint32_t j[4], float4 w, float4& v0, float4& v1) {
  float4 M[kSkinBoneRows];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t r = 0; r < kSkinBoneRows; ++r)
    M[r] = blend_row(w, bones[kSkinBoneRows * j[0] + r], bones[kSkinBoneRows * j[1] + r], bones[kSkinBoneRows * j[2] + r], bones[kSkinBoneRows * j[3] + r]);
  const float px = v0.x, py = v0.y, pz = v0.z, nx = v0.w, ny = v1.x, nz = v1.y;
  float p[kSkinBoneRows], n[kSkinBoneRows];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t r = 0; r < kSkinBoneRows; ++r) {
    p[r] = ((M[r].x * px + M[r].y * py) + M[r].z * pz) + M[r].w;
    n[r] = (M[r].x * nx + M[r].y * ny) + M[r].z * nz;
  }
  v0 = make_float4(p[0], p[1], p[2], n[0]);
  v1 = make_float4(n[1], n[2], v1.z, v1.w);
}

// ---- dual-quaternion blending ----
// A bone as the kernels of this mode read it: the unit quaternion of the matrix's 3 x 3 (x, y, z, w), then the dual part (dx, dy, dz, dw)
// that carries the translation, 32 bytes.  pack_bone_dq (once per bone per pose: it feeds the device upload and the host reference
// alike) makes it in float64 by the rule's bone conversion and rounds to float32 at the end.
constexpr uint32_t kSkinDqBoneRows = 2;
// The bone conversion of THE DUAL-QUATERNION RULE, of a matrix given as pack_bone's three rows: float64 throughout, the operations in
// the specification's order, rounded to float32 at the end.  Shepperd's branches pick the largest of w, x, y, z to divide by; a
// comparison with a NaN is false, so such a matrix takes the last branch.  Nothing is checked: a matrix that is no rotation gives the
// rule's image of it.  One definition for the host (pack_bone_dq) and for the device, where k_clip_bones makes a played skin's table
// (float64 sqrt and / are correctly rounded on both sides).
GLZ_POST_FN void bone_dual_quat(const float4 m[kSkinBoneRows], float4 rows[2]) {
  const double m00 = (double)m[0].x, m01 = (double)m[0].y, m02 = (double)m[0].z, m10 = (double)m[1].x, m11 = (double)m[1].y, m12 = (double)m[1].z, m20 = (double)m[2].x,
               m21 = (double)m[2].y, m22 = (double)m[2].z;
  const double tr = (m00 + m11) + m22;
  double x, y, z, w;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    w = s / 4.0;
    x = (m21 - m12) / s;
    y = (m02 - m20) / s;
    z = (m10 - m01) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = 2.0 * sqrt(((1.0 + m00) - m11) - m22);
    w = (m21 - m12) / s;
    x = s / 4.0;
    y = (m01 + m10) / s;
    z = (m02 + m20) / s;
  } else if (m11 > m22) {
    const double s = 2.0 * sqrt(((1.0 + m11) - m00) - m22);
    w = (m02 - m20) / s;
    x = (m01 + m10) / s;
    y = s / 4.0;
    z = (m12 + m21) / s;
  } else {
    const double s = 2.0 * sqrt(((1.0 + m22) - m00) - m11);
    w = (m10 - m01) / s;
    x = (m02 + m20) / s;
    y = (m12 + m21) / s;
    z = s / 4.0;
  }
  const double len = sqrt(((x * x + y * y) + z * z) + w * w);   // a uniform scale drops out here
  x = x / len;
  y = y / len;
  z = z / len;
  w = w / len;
  const double tx = (double)m[0].w, ty = (double)m[1].w, tz = (double)m[2].w;
  const double dx = 0.5 * ((tx * w + ty * z) - tz * y);
  const double dy = 0.5 * ((ty * w + tz * x) - tx * z);
  const double dz = 0.5 * ((tz * w + tx * y) - ty * x);
  const double dw = -0.5 * ((tx * x + ty * y) + tz * z);
  rows[0] = make_float4((float)x, (float)y, (float)z, (float)w);
  rows[1] = make_float4((float)dx, (float)dy, (float)dz, (float)dw);
}
inline void pack_bone_dq(const glz_transform& b, float4 rows[kSkinDqBoneRows]) {
  float4 m[kSkinBoneRows];
  pack_bone(b, m);
  bone_dual_quat(m, rows);
}
// float4 a bone of the table a skin's kernels read, by its blend mode (GLZ_SKIN_*)
inline uint32_t bone_rows(int blend) { return blend == GLZ_SKIN_DUAL_QUATERNION ? kSkinDqBoneRows : kSkinBoneRows; }

// One vertex, the arguments of skin_vertex; bones: kSkinDqBoneRows float4 per bone.  The pivot of the sign step is joint 0 whatever its
// weight; no term is skipped for a zero weight; a blend of squared length 0 is not special-cased (1 / sqrt(0) is inf, the vertex comes out
// non-finite).
template <class Rows>
GLZ_POST_FN void skin_vertex_dq(Rows bones, const uint32_t j[4], float4 w, float4& v0, float4& v1) {
  const float4 q0 = bones[kSkinDqBoneRows * j[0]], q1 = bones[kSkinDqBoneRows * j[1]], q2 = bones[kSkinDqBoneRows * j[2]], q3 = bones[kSkinDqBoneRows * j[3]];
  const float4 d0 = bones[kSkinDqBoneRows * j[0] + 1], d1 = bones[kSkinDqBoneRows * j[1] + 1], d2 = bones[kSkinDqBoneRows * j[2] + 1],
               d3 = bones[kSkinDqBoneRows * j[3] + 1];
  // signs: a bone on the other hemisphere from the pivot's enters with its weight negated (dot < 0: -0, +0 and NaN keep the weight)
  const float dot1 = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
  const float dot2 = ((q0.x * q2.x + q0.y * q2.y) + q0.z * q2.z) + q0.w * q2.w;
  const float dot3 = ((q0.x * q3.x + q0.y * q3.y) + q0.z * q3.z) + q0.w * q3.w;
  const float4 c = make_float4(w.x, dot1 < 0.0f ? -w.y : w.y, dot2 < 0.0f ? -w.z : w.z, dot3 < 0.0f ? -w.w : w.w);
  const float4 R = blend_row(c, q0, q1, q2, q3), D = blend_row(c, d0, d1, d2, d3);
  const float nn = ((R.x * R.x + R.y * R.y) + R.z * R.z) + R.w * R.w;
  const float inv = 1.0f / sqrtf(nn);
  const float rx = R.x * inv, ry = R.y * inv, rz = R.z * inv, rw = R.w * inv;
  const float dx = D.x * inv, dy = D.y * inv, dz = D.z * inv, dw = D.w * inv;
  const float tx = 2.0f * (((rw * dx - dw * rx) + ry * dz) - rz * dy);
  const float ty = 2.0f * (((rw * dy - dw * ry) + rz * dx) - rx * dz);
  const float tz = 2.0f * (((rw * dz - dw * rz) + rx * dy) - ry * dx);
  const float px = v0.x, py = v0.y, pz = v0.z, nx = v0.w, ny = v1.x, nz = v1.y;
  // rot(v) = v + 2 r_v x (r_v x v + r_w v)
  const float pax = (ry * pz - rz * py) + rw * px, pay = (rz * px - rx * pz) + rw * py, paz = (rx * py - ry * px) + rw * pz;
  const float pbx = ry * paz - rz * pay, pby = rz * pax - rx * paz, pbz = rx * pay - ry * pax;
  const float nax = (ry * nz - rz * ny) + rw * nx, nay = (rz * nx - rx * nz) + rw * ny, naz = (rx * ny - ry * nx) + rw * nz;
  const float nbx = ry * naz - rz * nay, nby = rz * nax - rx * naz, nbz = rx * nay - ry * nax;
  v0 = make_float4((px + 2.0f * pbx) + tx, (py + 2.0f * pby) + ty, (pz + 2.0f * pbz) + tz, nx + 2.0f * nbx);
  v1 = make_float4(ny + 2.0f * nby, nz + 2.0f * nbz, v1.z, v1.w);
}

// the reference on host arrays (skin_host.cpp): n vertices, 4 joints and 4 weights each, every joint below n_bones; out may be `bind` itself
void host_skin_dq(const glz_vertex* bind, const uint16_t* joints, const float* weights, size_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out);
void host_skin(const glz_vertex* bind, const uint16_t* joints, const float* weights, size_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out);

}  // namespace post
}  // namespace glz
