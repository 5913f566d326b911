// Skins, morph targets, normal sets, skeletons and clips of a scene on the device: their records, their checks and their launches.
#include "deformers.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <string>

#include "skin.h"

namespace glz {
namespace {

bool overlaps(uint64_t first, uint64_t n, uint64_t other_first, uint64_t other_n) { return first < other_first + other_n && other_first < first + n; }

// A record's own copy of the scene's vertices [first, first + host.size()), a skin's bind pose or a morph's base: from the host copy (a
// replica on another device), or device to device from what the scene holds now (the mirror may be behind it), which the host copy is
// then read from as well, for replicas made later
bool own_range(const Deformers::Sources& s, uint32_t first, bool replica, std::vector<glz_vertex>& host, DeviceBuffer<float4>& buffer, const char* what, Error& err) {
  static_assert(sizeof(glz_vertex) == 2 * sizeof(float4), "a vertex is two float4");
  const size_t n = 2 * host.size();
  if (replica) return hip_ok(buffer.upload(reinterpret_cast<const float4*>(host.data()), n, s.stream), what, err);
  const float4* range = s.vertices + 2 * (size_t)first;
  return hip_ok(hipMemcpyAsync(host.data(), range, sizeof(float4) * n, hipMemcpyDeviceToHost, s.stream), "read vertices", err) &&
         hip_ok(hipStreamSynchronize(s.stream), "read vertices", err) && hip_ok(buffer.alloc(n), what, err) &&
         hip_ok(hipMemcpyAsync(buffer.ptr, range, sizeof(float4) * n, hipMemcpyDeviceToDevice, s.stream), what, err);
}

bool upload_morph_weights(const glz_morph_weights& w, DeviceBuffer<float>& buffer, hipStream_t st, Error& err) {
  if (buffer.ptr == nullptr || buffer.count != w.n_targets) {
    if (!hip_ok(buffer.alloc(w.n_targets), "alloc morph weights", err)) return false;
  }
  return hip_ok(hipMemcpyAsync(buffer.ptr, w.weights, sizeof(float) * w.n_targets, hipMemcpyHostToDevice, st), "upload morph weights", err);
}

// The timing hooks' one measurement: every stage once, not timed; then each stage `reps` times between two device events; one wait for
// the stream; ms[k] = stage k's time divided by reps
template <size_t K>
bool time_launches(hipStream_t st, uint32_t reps, const char* who, const std::function<bool()> (&stages)[K], float* ms, Error& err) {
  Events<K + 1> t;
  if (!t.create(err)) return false;
  for (const auto& stage : stages)
    if (!stage()) return false;
  (void)hipEventRecord(t.ev[0], st);
  for (size_t k = 0; k < K; ++k) {
    for (uint32_t i = 0; i < reps; ++i)
      if (!stages[k]()) return false;
    (void)hipEventRecord(t.ev[k + 1], st);
  }
  if (!hip_ok(hipStreamSynchronize(st), who, err)) return false;
  for (size_t k = 0; k < K; ++k) {
    (void)hipEventElapsedTime(&ms[k], t.ev[k], t.ev[k + 1]);
    ms[k] /= (float)reps;
  }
  return true;
}

}  // namespace

// ---- skinned meshes ----

int Deformers::install_skin(const Sources& s, int id, SkinHost&& h, bool replica, Error& err) {
  Skin k;
  k.h = std::move(h);
  static_assert(sizeof(uint2) == 4 * sizeof(uint16_t), "four joints are one uint2");
  if (!own_range(s, k.h.first, replica, k.h.bind, k.bind, "bind pose", err) ||
      !hip_ok(k.joints.upload(reinterpret_cast<const uint2*>(k.h.joints.data()), k.h.n, s.stream), "upload joints", err) ||
      !hip_ok(k.weights.upload(reinterpret_cast<const float4*>(k.h.weights.data()), k.h.n, s.stream), "upload weights", err) ||
      !hip_ok(hipStreamSynchronize(s.stream), "add_skin", err))
    return -1;
  skins_.emplace(id, std::move(k));
  return id;
}

int Deformers::add_skin(const Sources& s, const glz_skin& k, Error& err) {
  auto refuse = [&](const char* why) {
    err.fail(GLZ_E_ARG, why);
    return -1;
  };
  if (!k.joints || !k.weights) return refuse("add_skin: joints or weights is null");
  if (k.n_vertices == 0 || (uint64_t)k.first_vertex + k.n_vertices > s.data.vertices.size()) return refuse("add_skin: no vertices, or a range past the scene's vertex count");
  if (k.n_bones == 0 || k.n_bones > 65536u) return refuse("add_skin: n_bones must be 1 .. 65536 (joints are 16 bits)");
  for (size_t i = 0; i < 4 * (size_t)k.n_vertices; ++i)
    if (k.joints[i] >= k.n_bones) return refuse("add_skin: a joint names a bone past n_bones");
  for (const auto& kv : skins_)
    if (overlaps(k.first_vertex, k.n_vertices, kv.second.h.first, kv.second.h.n)) return refuse("add_skin: the range overlaps an existing skin");
  for (const auto& kv : morphs_)
    if (kv.second.h.skin < 0 && overlaps(k.first_vertex, k.n_vertices, kv.second.h.first, kv.second.h.layout.n_vertices))
      return refuse("add_skin: the range overlaps a free-standing morph");
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return -1;
  SkinHost h;
  h.first = k.first_vertex;
  h.n = k.n_vertices;
  h.n_bones = k.n_bones;
  h.bind.resize(k.n_vertices);
  h.joints.assign(k.joints, k.joints + 4 * (size_t)k.n_vertices);
  h.weights.assign(k.weights, k.weights + 4 * (size_t)k.n_vertices);
  const int id = install_skin(s, next_skin_, std::move(h), false, err);
  if (id >= 0) ++next_skin_;
  return id;
}

bool Deformers::remove_skin(int id, Error& err) {
  const auto it = skins_.find(id);
  if (it == skins_.end()) return err.fail(GLZ_E_ARG, "remove_skin: no such skin");
  if (it->second.h.morph >= 0) return err.fail(GLZ_E_ARG, "remove_skin: the skin still carries a morph (remove_morph first)");
  if (it->second.h.skeleton >= 0) return err.fail(GLZ_E_ARG, "remove_skin: the skin still has a skeleton (remove_skeleton first)");
  skins_.erase(it);
  return true;
}

bool Deformers::set_skin_blend(int id, int blend, Error& err) {
  const auto it = skins_.find(id);
  if (it == skins_.end()) return err.fail(GLZ_E_ARG, "set_skin_blend: no such skin");
  if (blend != GLZ_SKIN_LINEAR && blend != GLZ_SKIN_DUAL_QUATERNION) return err.fail(GLZ_E_ARG, "set_skin_blend: unknown blend mode");
  it->second.h.blend = blend;   // no bones are kept between calls: the next pose packs its bones for this mode
  return true;
}

int Deformers::skin_blend(int id, Error& err) const {
  const auto it = skins_.find(id);
  if (it == skins_.end()) {
    err.fail(GLZ_E_ARG, "skin_blend: no such skin");
    return -1;
  }
  return it->second.h.blend;
}

// ---- morph targets ----

int Deformers::install_morph(const Sources& s, int id, MorphHost&& h, bool replica, Error& err) {
  Morph m;
  m.h = std::move(h);
  const post::MorphLayout& l = m.h.layout;
  if ((m.h.skin < 0 && !own_range(s, m.h.first, replica, m.h.base, m.base, "morph base", err)) ||
      !hip_ok(m.counts.upload(l.counts.data(), l.counts.size(), s.stream), "upload morph counts", err) ||
      !hip_ok(m.slices.upload(l.slices.data(), l.slices.size(), s.stream), "upload morph slices", err) ||
      !hip_ok(m.entries.upload(l.entries.data(), l.entries.size(), s.stream), "upload morph entries", err) || !hip_ok(hipStreamSynchronize(s.stream), "add_morph", err))
    return -1;
  if (m.h.skin >= 0) skins_.at(m.h.skin).h.morph = id;
  morphs_.emplace(id, std::move(m));
  return id;
}

int Deformers::add_morph(const Sources& s, const glz_morph& g, Error& err) {
  auto refuse = [&](const std::string& why) {
    err.fail(GLZ_E_ARG, "add_morph: " + why);
    return -1;
  };
  if (g.n_vertices == 0 || (uint64_t)g.first_vertex + g.n_vertices > s.data.vertices.size()) return refuse("no vertices, or a range past the scene's vertex count");
  if (g.skin >= 0) {
    const auto it = skins_.find(g.skin);
    if (it == skins_.end()) return refuse("no such skin");
    if (it->second.h.morph >= 0) return refuse("the skin already carries a morph");
    if (it->second.h.first != g.first_vertex || it->second.h.n != g.n_vertices) return refuse("an attached morph's range must be exactly its skin's");
  } else {
    if (g.skin != -1) return refuse("skin must be a skin's id, or -1");
    for (const auto& kv : skins_)
      if (overlaps(g.first_vertex, g.n_vertices, kv.second.h.first, kv.second.h.n)) return refuse("the range overlaps a skin");
    for (const auto& kv : morphs_)
      if (overlaps(g.first_vertex, g.n_vertices, kv.second.h.first, kv.second.h.layout.n_vertices)) return refuse("the range overlaps an existing morph");
  }
  MorphHost h;
  h.first = g.first_vertex;
  h.skin = g.skin;
  std::string why;
  if (!post::pack_morph(g.n_vertices, g.targets, g.n_targets, h.layout, why)) return refuse(why);
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return -1;
  if (g.skin < 0) h.base.resize(g.n_vertices);
  const int id = install_morph(s, next_morph_, std::move(h), false, err);
  if (id >= 0) ++next_morph_;
  return id;
}

bool Deformers::remove_morph(int id, Error& err) {
  const auto it = morphs_.find(id);
  if (it == morphs_.end()) return err.fail(GLZ_E_ARG, "remove_morph: no such morph");
  if (it->second.h.skin >= 0) {
    for (const auto& kv : clips_)   // (a clip's weight track feeds the fused kernel of this morph)
      if (!kv.second.h.morph_weights.empty() && skeletons_.at(kv.second.h.skeleton).h.skin == it->second.h.skin)
        return err.fail(GLZ_E_ARG, "remove_morph: a clip's weight track still drives the morph (remove_clip first)");
    skins_.at(it->second.h.skin).h.morph = -1;
  }
  morphs_.erase(it);
  return true;
}

// ---- animations ----

bool Deformers::animated_span(const glz_animation* anim, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string(who) + ": " + why); };
  if (!anim) return refuse("the animation is null");
  if (anim->n_morphs && !anim->morphs) return refuse("morphs is null");
  if (anim->n_poses ? !anim->poses : anim->n_morphs == 0) return refuse("poses is null or empty");
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < anim->n_poses; ++i) {
    const glz_pose& p = anim->poses[i];
    const auto it = skins_.find(p.skin);
    if (it == skins_.end()) return refuse("no such skin");
    if (!p.bones) return refuse("a pose's bones are null");
    if (p.n_bones != it->second.h.n_bones) return refuse("a pose's bone count is not its skin's");
    for (uint32_t k = 0; k < i; ++k)
      if (anim->poses[k].skin == p.skin) return refuse("a skin is named twice");
    lo = std::min<uint64_t>(lo, it->second.h.first);
    hi = std::max<uint64_t>(hi, (uint64_t)it->second.h.first + it->second.h.n);
  }
  for (uint32_t i = 0; i < anim->n_morphs; ++i) {
    const glz_morph_weights& w = anim->morphs[i];
    const auto it = morphs_.find(w.morph);
    if (it == morphs_.end()) return refuse("no such morph");
    const MorphHost& m = it->second.h;
    if (!w.weights) return refuse("a morph's weights are null");
    if (w.n_targets != m.layout.n_targets) return refuse("a morph's target count is not its morph's");
    for (uint32_t k = 0; k < i; ++k)
      if (anim->morphs[k].morph == w.morph) return refuse("a morph is named twice");
    if (m.skin >= 0) {   // no bones are kept between calls: the skin's pose must come with it
      bool posed = false;
      for (uint32_t k = 0; k < anim->n_poses; ++k) posed = posed || anim->poses[k].skin == m.skin;
      if (!posed) return refuse("an attached morph is named without its skin's pose");
    }
    lo = std::min<uint64_t>(lo, m.first);
    hi = std::max<uint64_t>(hi, (uint64_t)m.first + m.layout.n_vertices);
  }
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  return true;
}

bool Deformers::deform(const Morph* morph, const float* weights, const glz_pose* pose, std::vector<float4>* packed, DeviceBuffer<float4>* bones, float4* span,
                       uint32_t span_first, hipStream_t st, Error& err) const {
  if (pose) {   // the bones, packed for the skin's blend mode (post::bone_rows float4 a bone), on their way up
    const Skin& s = skins_.at(pose->skin);
    const bool dq = s.h.blend == GLZ_SKIN_DUAL_QUATERNION;
    const uint32_t rows = post::bone_rows(s.h.blend);
    packed->resize((size_t)rows * s.h.n_bones);
    for (uint32_t b = 0; b < s.h.n_bones; ++b) {
      if (dq) post::pack_bone_dq(pose->bones[b], packed->data() + (size_t)rows * b);
      else post::pack_bone(pose->bones[b], packed->data() + (size_t)rows * b);
    }
    if (bones->ptr == nullptr || bones->count != packed->size()) {
      if (!hip_ok(bones->alloc(packed->size()), "alloc bones", err)) return false;
    }
    if (!hip_ok(hipMemcpyAsync(bones->ptr, packed->data(), sizeof(float4) * packed->size(), hipMemcpyHostToDevice, st), "upload bones", err)) return false;
  }
  return deform_tables(morph, weights, pose ? &skins_.at(pose->skin) : nullptr, pose ? bones->ptr : nullptr, span, span_first, st, err);
}

bool Deformers::deform_tables(const Morph* morph, const float* weights, const Skin* skin, const float4* bones, float4* span, uint32_t span_first, hipStream_t st,
                              Error& err) const {
  MorphArgs m{};
  SkinArgs k{};
  const char* rule = "k_morph";   // which rule ran, for an error's text
  uint32_t first = 0;
  if (morph) {
    const post::MorphLayout& l = morph->h.layout;
    m = MorphArgs{morph->h.skin >= 0 ? skins_.at(morph->h.skin).bind.ptr : morph->base.ptr, morph->counts.ptr, morph->slices.ptr, morph->entries.ptr, l.n_vertices, weights, l.n_targets};
    first = morph->h.first;
  }
  if (skin) {
    const bool dq = skin->h.blend == GLZ_SKIN_DUAL_QUATERNION;
    k = SkinArgs{skin->bind.ptr, skin->joints.ptr, skin->weights.ptr, skin->h.n, bones, skin->h.n_bones, skin->h.blend};
    rule = dq ? (morph ? "k_morph_skin_dq" : "k_skin_dq") : (morph ? "k_morph_skin" : "k_skin");
    first = skin->h.first;
  }
  return hip_ok(launch_deform(st, morph ? &m : nullptr, skin ? &k : nullptr, span + 2 * (size_t)(first - span_first)), rule, err);
}

bool Deformers::animate_into(const glz_animation& anim, float4* span, uint32_t span_first, AnimationUploads& up, hipStream_t st, Error& err) const {
  up.packed.resize(anim.n_poses);
  up.bones.resize(anim.n_poses);
  up.weights.resize(anim.n_morphs);
  for (uint32_t i = 0; i < anim.n_morphs; ++i) {
    const Morph& m = morphs_.at(anim.morphs[i].morph);
    if (!upload_morph_weights(anim.morphs[i], up.weights[i], st, err)) return false;
    if (m.h.skin < 0 && !deform(&m, up.weights[i].ptr, nullptr, nullptr, nullptr, span, span_first, st, err)) return false;
  }
  for (uint32_t i = 0; i < anim.n_poses; ++i) {
    const int attached = skins_.at(anim.poses[i].skin).h.morph;
    uint32_t named = anim.n_morphs;   // where the skin's morph is named, if it is
    for (uint32_t k = 0; k < anim.n_morphs && attached >= 0; ++k)
      if (anim.morphs[k].morph == attached) named = k;
    const bool fused = named != anim.n_morphs;
    if (!deform(fused ? &morphs_.at(attached) : nullptr, fused ? up.weights[named].ptr : nullptr, &anim.poses[i], &up.packed[i], &up.bones[i], span, span_first, st, err))
      return false;
  }
  return true;
}

// ---- skeletons and clips ----

int Deformers::install_skeleton(const Sources& s, int id, SkeletonHost&& h, Error& err) {
  Skeleton k;
  k.h = std::move(h);
  const size_t n = k.h.n_bones;
  if (!hip_ok(k.parents.upload(k.h.parents.data(), n, s.stream), "upload parents", err) ||
      !hip_ok(k.level_bones.upload(k.h.level_bones.data(), k.h.level_bones.size(), s.stream), "upload levels", err) ||
      !hip_ok(k.level_offsets.upload(k.h.level_offsets.data(), k.h.level_offsets.size(), s.stream), "upload levels", err) ||
      !hip_ok(k.inverse_bind.upload(k.h.inverse_bind.data(), k.h.inverse_bind.size(), s.stream), "upload inverse bind", err) ||
      !hip_ok(k.world.alloc(post::kSkinBoneRows * n), "alloc world table", err) ||
      !hip_ok(k.bones.alloc(std::max(post::kSkinBoneRows, post::kSkinDqBoneRows) * n), "alloc bone table", err) || !hip_ok(hipStreamSynchronize(s.stream), "add_skeleton", err))
    return -1;
  skins_.at(k.h.skin).h.skeleton = id;
  skeletons_.emplace(id, std::move(k));
  return id;
}

int Deformers::add_skeleton(const Sources& s, const glz_skeleton& g, Error& err) {
  auto refuse = [&](const std::string& why) {
    err.fail(GLZ_E_ARG, "add_skeleton: " + why);
    return -1;
  };
  const auto it = skins_.find(g.skin);
  if (it == skins_.end()) return refuse("no such skin");
  if (it->second.h.skeleton >= 0) return refuse("the skin already has a skeleton");
  if (g.n_bones != it->second.h.n_bones) return refuse("n_bones is not the skin's");
  std::string why;
  if (!post::clip_check_skeleton(g.parents, g.inverse_bind, g.n_bones, why)) return refuse(why);
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return -1;
  SkeletonHost h;
  h.skin = g.skin;
  h.n_bones = g.n_bones;
  h.parents.assign(g.parents, g.parents + g.n_bones);
  h.inverse_bind.resize(post::kSkinBoneRows * ((size_t)g.n_bones + 1));
  for (uint32_t b = 0; b <= g.n_bones; ++b) {
    const post::Affine a = post::affine_of(b < g.n_bones ? g.inverse_bind[b] : g.root);
    std::copy(a.r, a.r + post::kSkinBoneRows, h.inverse_bind.begin() + post::kSkinBoneRows * (size_t)b);
  }
  post::clip_levels(g.parents, g.n_bones, h.level_bones, h.level_offsets);
  const int id = install_skeleton(s, next_skeleton_, std::move(h), err);
  if (id >= 0) ++next_skeleton_;
  return id;
}

bool Deformers::remove_skeleton(int id, Error& err) {
  const auto it = skeletons_.find(id);
  if (it == skeletons_.end()) return err.fail(GLZ_E_ARG, "remove_skeleton: no such skeleton");
  for (auto c = clips_.begin(); c != clips_.end();) c = c->second.h.skeleton == id ? clips_.erase(c) : std::next(c);
  skins_.at(it->second.h.skin).h.skeleton = -1;
  skeletons_.erase(it);
  return true;
}

int Deformers::install_clip(const Sources& s, int id, ClipHost&& h, Error& err) {
  Clip c;
  c.h = std::move(h);
  const Skeleton& k = skeletons_.at(c.h.skeleton);
  const bool scaled = !c.h.scales.empty(), tracked = !c.h.morph_weights.empty();
  if (!hip_ok(c.translations.upload(c.h.translations.data(), c.h.translations.size(), s.stream), "upload clip translations", err) ||
      !hip_ok(c.rotations.upload(c.h.rotations.data(), c.h.rotations.size(), s.stream), "upload clip rotations", err) ||
      (scaled && !hip_ok(c.scales.upload(c.h.scales.data(), c.h.scales.size(), s.stream), "upload clip scales", err)) ||
      (tracked && (!hip_ok(c.morph_weights.upload(c.h.morph_weights.data(), c.h.morph_weights.size(), s.stream), "upload clip morph weights", err) ||
                   !hip_ok(c.weights.alloc(c.h.n_targets), "alloc clip weight table", err))))
    return -1;
  const ClipArgs args{c.translations.ptr, c.rotations.ptr, c.scales.ptr, c.morph_weights.ptr, k.parents.ptr, k.level_bones.ptr, k.level_offsets.ptr, k.inverse_bind.ptr,
                      k.world.ptr,        k.bones.ptr,     c.weights.ptr, k.h.n_bones, (uint32_t)k.h.level_offsets.size() - 1, c.h.n_targets};
  if (!hip_ok(c.args.upload(&args, 1, s.stream), "upload clip", err) || !hip_ok(hipStreamSynchronize(s.stream), "add_clip", err)) return -1;
  clips_.emplace(id, std::move(c));
  return id;
}

int Deformers::add_clip(const Sources& s, const glz_clip& g, Error& err) {
  auto refuse = [&](const std::string& why) {
    err.fail(GLZ_E_ARG, "add_clip: " + why);
    return -1;
  };
  const auto it = skeletons_.find(g.skeleton);
  if (it == skeletons_.end()) return refuse("no such skeleton");
  std::string why;
  if (!post::clip_check_keys(g, why)) return refuse(why);
  if (g.morph_weights) {
    const int morph = skins_.at(it->second.h.skin).h.morph;
    if (morph < 0) return refuse("a weight track needs an attached morph on the skeleton's skin");
    if (g.n_targets != morphs_.at(morph).h.layout.n_targets) return refuse("the weight track's target count is not the morph's");
  }
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return -1;
  const size_t per_key = (size_t)g.n_keys * it->second.h.n_bones;
  ClipHost h;
  h.skeleton = g.skeleton;
  h.n_keys = g.n_keys;
  h.n_targets = g.n_targets;
  h.times.assign(g.times, g.times + g.n_keys);
  h.translations.assign(g.translations, g.translations + 3 * per_key);
  h.rotations.assign(g.rotations, g.rotations + 4 * per_key);
  if (g.scales) h.scales.assign(g.scales, g.scales + 3 * per_key);
  if (g.morph_weights) h.morph_weights.assign(g.morph_weights, g.morph_weights + (size_t)g.n_keys * g.n_targets);
  const int id = install_clip(s, next_clip_, std::move(h), err);
  if (id >= 0) ++next_clip_;
  return id;
}

bool Deformers::remove_clip(int id, Error& err) {
  if (clips_.erase(id) == 0) return err.fail(GLZ_E_ARG, "remove_clip: no such clip");
  return true;
}

bool Deformers::played_span(const glz_play* plays, uint32_t n, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string(who) + ": " + why); };
  if (!plays || n == 0) return refuse("plays is null or empty");
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = clips_.find(plays[i].clip);
    if (it == clips_.end()) return refuse("no such clip");
    if (!std::isfinite(plays[i].time)) return refuse("a time is not finite");
    for (uint32_t k = 0; k < i; ++k)
      if (clips_.at(plays[k].clip).h.skeleton == it->second.h.skeleton) return refuse("two plays name clips of the same skeleton");
    const SkinHost& skin = skins_.at(skeletons_.at(it->second.h.skeleton).h.skin).h;
    lo = std::min<uint64_t>(lo, skin.first);
    hi = std::max<uint64_t>(hi, (uint64_t)skin.first + skin.n);
  }
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  return true;
}

bool Deformers::upload_plays(const glz_play* plays, uint32_t n, PlayUploads& up, hipStream_t st, Error& err) const {
  up.records.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const Clip& c = clips_.at(plays[i].clip);
    const post::ClipKey key = post::clip_key(c.h.times.data(), c.h.n_keys, plays[i].time);
    up.records[i] = ClipPlay{c.args.ptr, key.k0, key.k1, key.u, skins_.at(skeletons_.at(c.h.skeleton).h.skin).h.blend};
  }
  if (up.table.ptr == nullptr || up.table.count != n) {
    if (!hip_ok(up.table.alloc(n), "alloc plays", err)) return false;
  }
  return hip_ok(hipMemcpyAsync(up.table.ptr, up.records.data(), sizeof(ClipPlay) * n, hipMemcpyHostToDevice, st), "upload plays", err);
}

bool Deformers::play_into(const glz_play* plays, uint32_t n, float4* span, uint32_t span_first, PlayUploads& up, hipStream_t st, Error& err) const {
  if (!upload_plays(plays, n, up, st, err) || !hip_ok(launch_clip_bones(st, up.table.ptr, n), "k_clip_bones", err)) return false;
  for (uint32_t i = 0; i < n; ++i) {
    const Clip& c = clips_.at(plays[i].clip);
    const Skeleton& k = skeletons_.at(c.h.skeleton);
    const Skin& skin = skins_.at(k.h.skin);
    const bool fused = c.weights.ptr != nullptr;   // (add_clip and remove_morph see to it that the morph is there)
    if (!deform_tables(fused ? &morphs_.at(skin.h.morph) : nullptr, c.weights.ptr, &skin, k.bones.ptr, span, span_first, st, err)) return false;
  }
  return true;
}

bool Deformers::clip_bones(const Sources& s, const glz_play& play, float* rows_out, float* weights_out, Error& err) const {
  uint32_t first = 0, count = 0;
  if (!rows_out) return err.fail(GLZ_E_ARG, "clip bones: null output");
  if (!played_span(&play, 1, "clip bones", first, count, err) || !hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return false;
  const Clip& c = clips_.at(play.clip);
  const Skeleton& k = skeletons_.at(c.h.skeleton);
  PlayUploads up;
  if (!upload_plays(&play, 1, up, s.stream, err) || !hip_ok(launch_clip_bones(s.stream, up.table.ptr, 1), "k_clip_bones", err)) return false;
  const size_t rows = (size_t)post::bone_rows(skins_.at(k.h.skin).h.blend) * k.h.n_bones;
  if (!hip_ok(hipMemcpyAsync(rows_out, k.bones.ptr, sizeof(float4) * rows, hipMemcpyDeviceToHost, s.stream), "read bone table", err)) return false;
  if (weights_out && c.weights.ptr &&
      !hip_ok(hipMemcpyAsync(weights_out, c.weights.ptr, sizeof(float) * c.h.n_targets, hipMemcpyDeviceToHost, s.stream), "read weight table", err))
    return false;
  return hip_ok(hipStreamSynchronize(s.stream), "clip bones", err);
}

// ---- vertex normals from deformed positions ----

bool Deformers::pack_normals(const Sources& s, const glz_normals& g, post::NormalLayout& layout, Error& err) const {
  auto refuse = [&](const std::string& why) { return err.fail(GLZ_E_ARG, "add_normals: " + why); };
  const SceneData& d = s.data;
  if (g.n_vertices == 0 || (uint64_t)g.first_vertex + g.n_vertices > d.vertices.size()) return refuse("no vertices, or a range past the scene's vertex count");
  for (const auto& kv : normals_)
    if (overlaps(g.first_vertex, g.n_vertices, kv.second.layout.first, kv.second.layout.n_vertices)) return refuse("the range overlaps an existing normal set");
  std::string why;
  return post::pack_normals(d.indices.data(), d.indices.size(), d.meshes.data(), d.meshes.size(), d.vertices.size(), g.first_vertex, g.n_vertices, g.groups, layout, why) ||
         refuse(why);
}

int Deformers::install_normals(const Sources& src, int id, post::NormalLayout&& layout, Error& err) {
  hipStream_t st = src.stream;
  NormalSet s;
  s.layout = std::move(layout);
  if (!hip_ok(s.faces.upload(s.layout.faces.data(), s.layout.faces.size(), st), "upload normal faces", err) ||
      !hip_ok(s.counts.upload(s.layout.counts.data(), s.layout.counts.size(), st), "upload normal counts", err) ||
      !hip_ok(s.slices.upload(s.layout.slices.data(), s.layout.slices.size(), st), "upload normal slices", err) ||
      !hip_ok(s.rows.upload(s.layout.rows.data(), s.layout.rows.size(), st), "upload normal rows", err) ||
      !hip_ok(s.face_vectors.alloc(std::max<size_t>(s.layout.n_faces, 1)), "alloc face vectors", err) || !hip_ok(hipStreamSynchronize(st), "add_normals", err))
    return -1;
  normals_.emplace(id, std::move(s));
  return id;
}

int Deformers::install_normals(const Sources& s, post::NormalLayout&& layout, Error& err) {
  const int id = install_normals(s, next_normals_, std::move(layout), err);
  if (id >= 0) ++next_normals_;
  return id;
}

bool Deformers::remove_normals(int id, Error& err) {
  if (normals_.erase(id) == 0) return err.fail(GLZ_E_ARG, "remove_normals: no such normal set");
  return true;
}

bool Deformers::run_normals(const Sources& src, int only, uint32_t& first, uint32_t& count, bool& ran, Error& err) const {
  uint64_t lo = first, hi = (uint64_t)first + count;
  const uint64_t written_lo = lo, written_hi = hi;
  ran = false;
  for (const auto& kv : normals_) {
    const NormalSet& s = kv.second;
    // (the rule is a function of positions alone: the whole set again, and what did not change comes out with the bits it had)
    if (s.layout.n_faces == 0 || (only >= 0 ? kv.first != only : s.layout.reach_lo >= written_hi || s.layout.reach_hi < written_lo)) continue;
    const NormalArgs a = normal_args(s);
    float4* range = src.vertices + 2 * (size_t)s.layout.first;
    if (!hip_ok(launch_face_vectors(src.stream, src.vertices, a, s.face_vectors.ptr), "k_face_vectors", err) ||
        !hip_ok(launch_vertex_normals(src.stream, range, a, s.face_vectors.ptr, range), "k_vertex_normals", err))
      return false;
    lo = std::min<uint64_t>(lo, s.layout.first);
    hi = std::max<uint64_t>(hi, (uint64_t)s.layout.first + s.layout.n_vertices);
    ran = true;
  }
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  return true;
}

// ---- replicas ----

bool Deformers::copy_from(const Sources& s, const Deformers& src, Error& err) {
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return false;
  for (const auto& kv : src.skins_) {
    SkinHost h = kv.second.h;
    h.morph = h.skeleton = -1;   // (its morph and its skeleton attach themselves below)
    if (install_skin(s, kv.first, std::move(h), true, err) < 0) return false;
  }
  for (const auto& kv : src.morphs_)
    if (install_morph(s, kv.first, MorphHost(kv.second.h), true, err) < 0) return false;
  for (const auto& kv : src.normals_)
    if (install_normals(s, kv.first, post::NormalLayout(kv.second.layout), err) < 0) return false;
  for (const auto& kv : src.skeletons_)
    if (install_skeleton(s, kv.first, SkeletonHost(kv.second.h), err) < 0) return false;
  for (const auto& kv : src.clips_)
    if (install_clip(s, kv.first, ClipHost(kv.second.h), err) < 0) return false;
  next_skeleton_ = src.next_skeleton_;
  next_clip_ = src.next_clip_;
  next_skin_ = src.next_skin_;
  next_morph_ = src.next_morph_;
  next_normals_ = src.next_normals_;
  return true;
}

// ---- timing hooks ----

bool Deformers::time_skin(const Sources& s, const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const {
  uint32_t first = 0, count = 0;
  if (!kernel_ms || reps == 0) return err.fail(GLZ_E_ARG, "skin timing: null output or no repeats");
  const glz_animation one{nullptr, 0, &pose, 1};
  if (!animated_span(&one, "skin timing", first, count, err)) return false;
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return false;
  std::vector<float4> packed;
  DeviceBuffer<float4> bones, out;
  if (!hip_ok(out.alloc(2 * (size_t)count), "alloc", err)) return false;
  return time_launches(s.stream, reps, "skin timing", {[&] { return deform(nullptr, nullptr, &pose, &packed, &bones, out.ptr, first, s.stream, err); }}, kernel_ms, err);
}

bool Deformers::time_clip(const Sources& s, const glz_play* plays, uint32_t n, uint32_t reps, float* kernel_ms, Error& err) const {
  uint32_t first = 0, count = 0;
  if (!kernel_ms || reps == 0) return err.fail(GLZ_E_ARG, "clip timing: null output or no repeats");
  if (!played_span(plays, n, "clip timing", first, count, err) || !hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return false;
  PlayUploads up;
  if (!upload_plays(plays, n, up, s.stream, err)) return false;
  return time_launches(s.stream, reps, "clip timing", {[&] { return hip_ok(launch_clip_bones(s.stream, up.table.ptr, n), "k_clip_bones", err); }}, kernel_ms, err);
}

bool Deformers::time_morph(const Sources& s, const glz_animation& one, uint32_t reps, float* kernel_ms, uint64_t* bytes, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string("morph timing: ") + why); };
  if (!kernel_ms || reps == 0) return refuse("null output or no repeats");
  if (!one.morphs || one.n_morphs != 1 || one.n_poses > 1) return refuse("one morph, alone or with its skin's pose");
  const bool fused = one.n_poses == 1;
  const glz_morph_weights& w = one.morphs[0];
  uint32_t first = 0, count = 0;
  if (fused && !animated_span(&one, "morph timing", first, count, err)) return false;
  const auto it = morphs_.find(w.morph);
  if (it == morphs_.end() || !w.weights || w.n_targets != it->second.h.layout.n_targets) return refuse("no such morph, null weights, or a target count that is not the morph's");
  const Morph& m = it->second;
  const post::MorphLayout& l = m.h.layout;
  if (fused && m.h.skin != one.poses[0].skin) return refuse("the pose is not of the morph's skin");
  if (!hip_ok(hipSetDevice(s.device), "hipSetDevice", err)) return false;
  std::vector<float4> packed;
  DeviceBuffer<float4> bones, out;
  DeviceBuffer<float> weights;
  if (!hip_ok(out.alloc(2 * (size_t)l.n_vertices), "alloc", err)) return false;
  auto once = [&] {
    return upload_morph_weights(w, weights, s.stream, err) && deform(&m, weights.ptr, fused ? one.poses : nullptr, &packed, &bones, out.ptr, m.h.first, s.stream, err);
  };
  if (!time_launches(s.stream, reps, "morph timing", {once}, kernel_ms, err)) return false;
  if (bytes) {
    *bytes = (uint64_t)l.n_vertices * (32 + 32 + 4) + (uint64_t)l.slices.size() * 8 + l.n_entries * 32 + (uint64_t)l.n_targets * 4;
    if (fused) *bytes += (uint64_t)l.n_vertices * (8 + 16) + (uint64_t)skins_.at(m.h.skin).h.n_bones * sizeof(float4) * post::bone_rows(skins_.at(m.h.skin).h.blend);
  }
  return true;
}

bool Deformers::time_normals(const Sources& src, int id, uint32_t reps, float ms[2], uint64_t bytes[2], Error& err) const {
  const auto it = normals_.find(id);
  if (!ms || reps == 0 || it == normals_.end()) return err.fail(GLZ_E_ARG, "normals timing: null output, no repeats, or no such normal set");
  const NormalSet& s = it->second;
  if (!hip_ok(hipSetDevice(src.device), "hipSetDevice", err)) return false;
  hipStream_t st = src.stream;
  DeviceBuffer<float4> face_vectors, out;
  const NormalArgs a = normal_args(s);
  const float4* range = src.vertices + 2 * (size_t)s.layout.first;
  if (!hip_ok(face_vectors.alloc(std::max<size_t>(s.layout.n_faces, 1)), "alloc", err) || !hip_ok(out.alloc(2 * (size_t)s.layout.n_vertices), "alloc", err) ||
      !hip_ok(hipMemcpyAsync(out.ptr, range, sizeof(float4) * 2 * (size_t)s.layout.n_vertices, hipMemcpyDeviceToDevice, st), "copy vertices", err))
    return false;
  if (!time_launches(st, reps, "normals timing",
                     {[&] { return hip_ok(launch_face_vectors(st, src.vertices, a, face_vectors.ptr), "k_face_vectors", err); },
                      [&] { return hip_ok(launch_vertex_normals(st, range, a, face_vectors.ptr, out.ptr), "k_vertex_normals", err); }},
                     ms, err))
    return false;
  if (bytes) {
    uint64_t with_faces = 0;
    for (uint32_t c : s.layout.counts) with_faces += c != 0;
    bytes[0] = (uint64_t)s.layout.n_faces * (12 + 3 * 16 + 16);
    bytes[1] = (uint64_t)s.layout.n_vertices * 4 + (uint64_t)s.layout.slices.size() * 8 + s.layout.n_entries * (4 + 16) + with_faces * (32 + 12);
  }
  return true;
}

}  // namespace glz
