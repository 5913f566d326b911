// glz_host_skin: the skinning rule of skin.h on the host cores, no device -- the reference k_skin is compared with bit for bit.
// glz_host_skin_dq: the same for the dual-quaternion rule and k_skin_dq (the bone conversion both sides share is skin.h's bone_dual_quat).
#include "skin.h"

#include <vector>

namespace glz {
namespace post {

void host_skin(const glz_vertex* bind, const uint16_t* joints, const float* weights, size_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out) {
  std::vector<float4> rows((size_t)kSkinBoneRows * n_bones);
  for (uint32_t b = 0; b < n_bones; ++b) pack_bone(bones[b], rows.data() + (size_t)kSkinBoneRows * b);
  for (size_t i = 0; i < n; ++i) {
    const glz_vertex& v = bind[i];
    const uint32_t j[4] = {joints[4 * i], joints[4 * i + 1], joints[4 * i + 2], joints[4 * i + 3]};
    const float4 w = make_float4(weights[4 * i], weights[4 * i + 1], weights[4 * i + 2], weights[4 * i + 3]);
    float4 v0 = make_float4(v.vv[0], v.vv[1], v.vv[2], v.vn[0]), v1 = make_float4(v.vn[1], v.vn[2], v.vt[0], v.vt[1]);
    skin_vertex(rows.data(), j, w, v0, v1);
    out[i] = glz_vertex{{v0.x, v0.y, v0.z}, {v0.w, v1.x, v1.y}, {v1.z, v1.w}};
  }
}

void host_skin_dq(const glz_vertex* bind, const uint16_t* joints, const float* weights, size_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out) {
  std::vector<float4> rows((size_t)kSkinDqBoneRows * n_bones);
  for (uint32_t b = 0; b < n_bones; ++b) pack_bone_dq(bones[b], rows.data() + (size_t)kSkinDqBoneRows * b);
  for (size_t i = 0; i < n; ++i) {
    const glz_vertex& v = bind[i];
    const uint32_t j[4] = {joints[4 * i], joints[4 * i + 1], joints[4 * i + 2], joints[4 * i + 3]};
    const float4 w = make_float4(weights[4 * i], weights[4 * i + 1], weights[4 * i + 2], weights[4 * i + 3]);
    float4 v0 = make_float4(v.vv[0], v.vv[1], v.vv[2], v.vn[0]), v1 = make_float4(v.vn[1], v.vn[2], v.vt[0], v.vt[1]);
    skin_vertex_dq(rows.data(), j, w, v0, v1);
    out[i] = glz_vertex{{v0.x, v0.y, v0.z}, {v0.w, v1.x, v1.y}, {v1.z, v1.w}};
  }
}

}  // namespace post
}  // namespace glz
