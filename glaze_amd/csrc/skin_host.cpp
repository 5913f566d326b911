// glz_host_skin: the skinning rule of skin.h on the host cores, no device -- the reference k_skin is compared with bit for bit.
// glz_host_skin_dq, glz_host_bone_dual_quats: the same for the dual-quaternion rule and k_skin_dq, and the bone conversion both sides share.
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

// The bone conversion of THE DUAL-QUATERNION RULE: float64 throughout, the operations in the specification's order, rounded to float32
// at the end.  Shepperd's branches pick the largest of w, x, y, z to divide by; a comparison with a NaN is false, so such a matrix takes
// the last branch.  Nothing is checked: a matrix that is no rotation gives the rule's image of it.
void pack_bone_dq(const glz_transform& b, float4 rows[kSkinDqBoneRows]) {
  auto m = [&](int r, int c) { return (double)b.m[4 * c + r]; };
  const double m00 = m(0, 0), m11 = m(1, 1), m22 = m(2, 2);
  const double tr = (m00 + m11) + m22;
  double x, y, z, w;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    w = s / 4.0;
    x = (m(2, 1) - m(1, 2)) / s;
    y = (m(0, 2) - m(2, 0)) / s;
    z = (m(1, 0) - m(0, 1)) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = 2.0 * sqrt(((1.0 + m00) - m11) - m22);
    w = (m(2, 1) - m(1, 2)) / s;
    x = s / 4.0;
    y = (m(0, 1) + m(1, 0)) / s;
    z = (m(0, 2) + m(2, 0)) / s;
  } else if (m11 > m22) {
    const double s = 2.0 * sqrt(((1.0 + m11) - m00) - m22);
    w = (m(0, 2) - m(2, 0)) / s;
    x = (m(0, 1) + m(1, 0)) / s;
    y = s / 4.0;
    z = (m(1, 2) + m(2, 1)) / s;
  } else {
    const double s = 2.0 * sqrt(((1.0 + m22) - m00) - m11);
    w = (m(1, 0) - m(0, 1)) / s;
    x = (m(0, 2) + m(2, 0)) / s;
    y = (m(1, 2) + m(2, 1)) / s;
    z = s / 4.0;
  }
  const double len = sqrt(((x * x + y * y) + z * z) + w * w);   // a uniform scale drops out here
  x = x / len;
  y = y / len;
  z = z / len;
  w = w / len;
  const double tx = m(0, 3), ty = m(1, 3), tz = m(2, 3);
  const double dx = 0.5 * ((tx * w + ty * z) - tz * y);
  const double dy = 0.5 * ((ty * w + tz * x) - tx * z);
  const double dz = 0.5 * ((tz * w + tx * y) - ty * x);
  const double dw = -0.5 * ((tx * x + ty * y) + tz * z);
  rows[0] = make_float4((float)x, (float)y, (float)z, (float)w);
  rows[1] = make_float4((float)dx, (float)dy, (float)dz, (float)dw);
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
