// Linear-blend skinning (glz_renderer_pose_skins, glz_host_skin; include/glaze_abi.h holds the specification): one vertex under four
// weighted bones, in the ONE form both the host reference (skin_host.cpp; g++) and the device kernel (kernels_skin.hip; hipcc) compile:
// the same operations in the same order, -ffp-contract=off on both sides, so the two agree bit for bit.  Only + and *, float32.
//
// The normal goes through the blended matrix's 3 x 3 as it is -- not through its inverse transpose, and it is not renormalised (shading
// normalises the normal it interpolates).  That is EXACT ONLY FOR RIGID BONES (rotation + translation) blended with weights that sum to 1;
// under scale, shear or other weights the normal is the blended matrix's image of the bind normal, no more.
#pragma once
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

// the reference on host arrays (skin_host.cpp): n vertices, 4 joints and 4 weights each, every joint below n_bones; out may be `bind` itself
void host_skin(const glz_vertex* bind, const uint16_t* joints, const float* weights, size_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out);

}  // namespace post
}  // namespace glz
