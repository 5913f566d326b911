// Skeletons and clips (glz_renderer_play, glz_host_clip_bones; include/glaze_abi.h holds the specification, "THE CLIP RULE"): one bone of a
// keyframed clip from its two keys to its matrix, in the ONE form both the host reference (clip_host.cpp; g++) and the device kernel
// (kernels_clip.hip; hipcc) compile: the same operations in the same order, -ffp-contract=off on both sides, so the two agree bit for
// bit.  float32, + - x, one sqrtf and one 1.0f / x a bone, both correctly rounded on either side (skin.h and normals.h normalise the same
// way).  The key choice is the host's alone (clip_key): the kernel receives (k0, k1, u), never a time.
#pragma once
#include <math.h>

#include <string>
#include <vector>

#include "denoise.h"

namespace glz {
namespace post {

// An affine 3 x 4 as three rows of four, the layout of a linear skin's bone (pack_bone): r[i] = (M[i][0], M[i][1], M[i][2], M[i][3])
struct Affine {
  float4 r[3];
};

// the upper 3 x 4 of a column-major glz_transform
inline Affine affine_of(const glz_transform& t) {
  Affine a;
  for (int r = 0; r < 3; ++r) a.r[r] = make_float4(t.m[r], t.m[4 + r], t.m[8 + r], t.m[12 + r]);
  return a;
}

// The two keys of a play and the weight of the second (step 1 of the rule, made on the host in float32)
struct ClipKey {
  uint32_t k0, k1;
  float u;
};
// times: n >= 1 of them, finite and strictly ascending; t finite
inline ClipKey clip_key(const float* times, uint32_t n, float t) {
  if (t <= times[0]) return ClipKey{0, 0, 0.0f};
  if (t >= times[n - 1]) return ClipKey{n - 1, n - 1, 0.0f};
  uint32_t k0 = 0;
  while (times[k0 + 1] <= t) ++k0;   // the largest k with times[k] <= t; k0 + 1 <= n - 1 since t < times[n - 1]
  return ClipKey{k0, k0 + 1, (t - times[k0]) / (times[k0 + 1] - times[k0])};
}

// step 2: no term is skipped (u = 0 gives a + 0 x (b - a))
GLZ_POST_FN float clip_lerp(float a, float b, float u) { return a + u * (b - a); }

// steps 2 - 4: bone b's local matrix from its two keys.  translations / scales: 3 floats a bone a key, rotations: 4 (x, y, z, w), key
// after key; scales may be null: every scale is 1, and the product with it is still formed.
template <class Floats>
GLZ_POST_FN Affine clip_local(Floats translations, Floats rotations, Floats scales, bool scaled, uint32_t n_bones, uint32_t b, uint32_t k0, uint32_t k1, float u) {
  const size_t i0 = (size_t)k0 * n_bones + b, i1 = (size_t)k1 * n_bones + b;
  const float tx = clip_lerp(translations[3 * i0], translations[3 * i1], u), ty = clip_lerp(translations[3 * i0 + 1], translations[3 * i1 + 1], u),
              tz = clip_lerp(translations[3 * i0 + 2], translations[3 * i1 + 2], u);
  float sx = 1.0f, sy = 1.0f, sz = 1.0f;
  if (scaled) {
    sx = clip_lerp(scales[3 * i0], scales[3 * i1], u);
    sy = clip_lerp(scales[3 * i0 + 1], scales[3 * i1 + 1], u);
    sz = clip_lerp(scales[3 * i0 + 2], scales[3 * i1 + 2], u);
  }
  const float ax = rotations[4 * i0], ay = rotations[4 * i0 + 1], az = rotations[4 * i0 + 2], aw = rotations[4 * i0 + 3];
  float bx = rotations[4 * i1], by = rotations[4 * i1 + 1], bz = rotations[4 * i1 + 2], bw = rotations[4 * i1 + 3];
  // the hemisphere step: b enters negated if dot < 0 (-0, +0 and NaN keep it)
  const float dot = ((ax * bx + ay * by) + az * bz) + aw * bw;
  if (dot < 0.0f) {
    bx = -bx;
    by = -by;
    bz = -bz;
    bw = -bw;
  }
  const float Qx = clip_lerp(ax, bx, u), Qy = clip_lerp(ay, by, u), Qz = clip_lerp(az, bz, u), Qw = clip_lerp(aw, bw, u);
  const float nn = ((Qx * Qx + Qy * Qy) + Qz * Qz) + Qw * Qw;
  const float inv = 1.0f / sqrtf(nn);
  const float x = Qx * inv, y = Qy * inv, z = Qz * inv, w = Qw * inv;
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  Affine L;
  L.r[0] = make_float4((1.0f - 2.0f * (yy + zz)) * sx, (2.0f * (xy - wz)) * sy, (2.0f * (xz + wy)) * sz, tx);
  L.r[1] = make_float4((2.0f * (xy + wz)) * sx, (1.0f - 2.0f * (xx + zz)) * sy, (2.0f * (yz - wx)) * sz, ty);
  L.r[2] = make_float4((2.0f * (xz - wy)) * sx, (2.0f * (yz + wx)) * sy, (1.0f - 2.0f * (xx + yy)) * sz, tz);
  return L;
}

// step 5: C = A o B
GLZ_POST_FN float4 affine_row(float4 a, const Affine& B) {
  return make_float4((a.x * B.r[0].x + a.y * B.r[1].x) + a.z * B.r[2].x, (a.x * B.r[0].y + a.y * B.r[1].y) + a.z * B.r[2].y,
                     (a.x * B.r[0].z + a.y * B.r[1].z) + a.z * B.r[2].z, ((a.x * B.r[0].w + a.y * B.r[1].w) + a.z * B.r[2].w) + a.w);
}
GLZ_POST_FN Affine affine_product(const Affine& A, const Affine& B) {
  Affine C;
  C.r[0] = affine_row(A.r[0], B);
  C.r[1] = affine_row(A.r[1], B);
  C.r[2] = affine_row(A.r[2], B);
  return C;
}

// A skeleton's level table: the bones grouped by depth (level 0: the roots), in ascending bone order inside a level.  bones: n of them;
// offsets: levels + 1, level l is bones[offsets[l] .. offsets[l + 1]).  parents: checked (-1, or below the bone's own index).
void clip_levels(const int32_t* parents, uint32_t n, std::vector<uint32_t>& bones, std::vector<uint32_t>& offsets);
// What a skeleton and a clip must be wherever they come from (add_skeleton, add_clip, glz_host_clip_bones); false with the reason
bool clip_check_skeleton(const int32_t* parents, const glz_transform* inverse_bind, uint32_t n_bones, std::string& why);
bool clip_check_keys(const glz_clip& clip, std::string& why);
// The reference on host arrays (clip_host.cpp): steps 1 - 6 for every bone, the weight track (if weights_out is not null) lerped per
// target.  bones_out: n_bones matrices with the fourth row (0, 0, 0, 1).  Both arguments checked.
void host_clip_bones(const glz_skeleton& skeleton, const glz_clip& clip, float time, glz_transform* bones_out, float* weights_out);

}  // namespace post
}  // namespace glz
