// glz_host_clip_bones: THE CLIP RULE of clip.h on the host cores, no device -- the reference k_clip_bones is compared with bit for bit --
// and what add_skeleton / add_clip share with it: the checks and the level table.
#include "clip.h"

#include <algorithm>
#include <cmath>

namespace glz {
namespace post {

void clip_levels(const int32_t* parents, uint32_t n, std::vector<uint32_t>& bones, std::vector<uint32_t>& offsets) {
  std::vector<uint32_t> depth(n);
  uint32_t levels = 0;
  for (uint32_t b = 0; b < n; ++b) {   // parents come before children
    depth[b] = parents[b] < 0 ? 0 : depth[parents[b]] + 1;
    levels = std::max(levels, depth[b] + 1);
  }
  offsets.assign(levels + 1, 0);
  for (uint32_t b = 0; b < n; ++b) ++offsets[depth[b] + 1];
  for (uint32_t l = 0; l < levels; ++l) offsets[l + 1] += offsets[l];
  bones.resize(n);
  std::vector<uint32_t> next(offsets.begin(), offsets.end() - 1);
  for (uint32_t b = 0; b < n; ++b) bones[next[depth[b]]++] = b;   // ascending bone order inside a level
}

bool clip_check_skeleton(const int32_t* parents, const glz_transform* inverse_bind, uint32_t n_bones, std::string& why) {
  if (n_bones == 0) return why = "n_bones is 0", false;
  if (!parents || !inverse_bind) return why = "parents or inverse_bind is null", false;
  for (uint32_t b = 0; b < n_bones; ++b)
    if (parents[b] < -1 || (parents[b] >= 0 && (uint32_t)parents[b] >= b)) return why = "a parent must be -1 or below its bone's index", false;
  return true;
}

bool clip_check_keys(const glz_clip& clip, std::string& why) {
  if (clip.n_keys == 0) return why = "n_keys is 0", false;
  if (!clip.times || !clip.translations || !clip.rotations) return why = "times, translations or rotations is null", false;
  for (uint32_t k = 0; k < clip.n_keys; ++k)
    if (!std::isfinite(clip.times[k]) || (k > 0 && !(clip.times[k] > clip.times[k - 1]))) return why = "times must be finite and strictly ascending", false;
  if ((clip.morph_weights != nullptr) != (clip.n_targets != 0)) return why = "a weight track needs n_targets, and n_targets a weight track", false;
  return true;
}

void host_clip_bones(const glz_skeleton& sk, const glz_clip& clip, float time, glz_transform* bones_out, float* weights_out) {
  const ClipKey key = clip_key(clip.times, clip.n_keys, time);
  const Affine root = affine_of(sk.root);
  std::vector<Affine> world(sk.n_bones);
  for (uint32_t b = 0; b < sk.n_bones; ++b) {   // parents come before children: one pass in bone order
    const Affine L = clip_local(clip.translations, clip.rotations, clip.scales, clip.scales != nullptr, sk.n_bones, b, key.k0, key.k1, key.u);
    world[b] = affine_product(sk.parents[b] < 0 ? root : world[sk.parents[b]], L);
    const Affine B = affine_product(world[b], affine_of(sk.inverse_bind[b]));
    glz_transform& out = bones_out[b];
    for (int r = 0; r < 3; ++r) {
      out.m[r] = B.r[r].x;
      out.m[4 + r] = B.r[r].y;
      out.m[8 + r] = B.r[r].z;
      out.m[12 + r] = B.r[r].w;
    }
    out.m[3] = out.m[7] = out.m[11] = 0.0f;
    out.m[15] = 1.0f;
  }
  if (weights_out && clip.morph_weights)
    for (uint32_t t = 0; t < clip.n_targets; ++t)
      weights_out[t] = clip_lerp(clip.morph_weights[(size_t)key.k0 * clip.n_targets + t], clip.morph_weights[(size_t)key.k1 * clip.n_targets + t], key.u);
}

}  // namespace post
}  // namespace glz
