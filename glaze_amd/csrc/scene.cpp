// RayTraceInstance::new / RayTraceScene::new on HIP (lib/src/vulkan/instance.rs:376-427,
// lib/src/vulkan/scene.rs:1414-1556 and the helpers it calls).
#include "scene.h"

#include <algorithm>
#include <cmath>

#include "host_math.h"
#include "mipchain.h"
#include "skin.h"

namespace glz {

Instance::~Instance() {
  if (stream) (void)hipStreamDestroy(stream);
}

Instance* Instance::create(int hip_device, Error& err) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    err.fail(GLZ_E_DEVICE, "no HIP device available");
    return nullptr;
  }
  int chosen = -1;
  std::string arch;
  auto arch_of = [](int d) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) != hipSuccess) return std::string();
    return std::string(p.gcnArchName);
  };
  if (hip_device >= 0) {
    if (hip_device >= count) {
      err.fail(GLZ_E_ARG, "HIP device ordinal out of range");
      return nullptr;
    }
    chosen = hip_device;
    arch = arch_of(chosen);
  } else {
    for (int d = 0; d < count; ++d) {
      std::string a = arch_of(d);
      if (a.rfind("gfx950", 0) == 0) {
        chosen = d;
        arch = a;
        break;
      }
    }
  }
  // the code object is built for gfx950 only: any other device cannot run it (no fallback)
  if (chosen < 0 || arch.rfind("gfx950", 0) != 0) {
    err.fail(GLZ_E_DEVICE, "no gfx950 (MI355X) device found" + (arch.empty() ? std::string() : " (device is " + arch + ")"));
    return nullptr;
  }
  if (!hip_ok(hipSetDevice(chosen), "hipSetDevice", err)) return nullptr;
  Instance* inst = new Instance();
  inst->device = chosen;
  inst->arch = arch;
  if (!hip_ok(hipStreamCreateWithFlags(&inst->stream, hipStreamNonBlocking), "hipStreamCreate", err)) {
    delete inst;
    return nullptr;
  }
  return inst;
}

// References between the parts of a scene description, so that no kernel can index out of bounds
static bool valid_references(const SceneData& d, Error& err) {
  if (!valid_geometry(d, d.transforms.size(), err)) return false;
  for (const glz_mesh& m : d.meshes) {
    if (m.index_count % 3 != 0) return err.fail(GLZ_E_INVALID_DATA, "mesh index range outside the index buffer");
    if (m.material >= d.materials.size()) return err.fail(GLZ_E_INVALID_DATA, "mesh references a missing material");
  }
  auto tex_ok = [&](uint32_t id) { return id < d.textures.size(); };
  for (const glz_material& m : d.materials)
    if (!tex_ok(m.diffuse) || !tex_ok(m.roughness) || !tex_ok(m.metalness) || !tex_ok(m.normal) || !tex_ok(m.opacity))
      return err.fail(GLZ_E_INVALID_DATA, "material references a missing texture");
  return true;
}

// The one writer of `dev`: the view from nothing, each part's fields by the part that owns them
void Scene::compose() {
  dev = DeviceScene{};
  dev.vertices = geometry_.vertices.ptr;
  dev.indices = geometry_.indices.ptr;
  dev.instances = geometry_.instances.ptr;
  dev.transforms = geometry_.transforms.ptr;
  dev.derivatives = geometry_.derivatives.ptr;
  dev.srgb_lut = geometry_.srgb_lut.ptr;
  textures_.describe(dev);
  tables_.describe(dev);
  accel_.describe(dev);
  accel_.describe(info);
}

struct Scene::Composed {
  Scene& s;
  ~Composed() { s.compose(); }
};

Scene* Scene::create(Instance* inst, SceneData&& data, Error& err) {
  std::unique_ptr<Scene> s(new Scene());
  s->instance = inst;
  s->data = std::move(data);
  SceneData& d = s->data;
  // defaults for absent pieces (scene.rs:1427-1434, :1467-1469; Texture::default is texture 0)
  if (d.transforms.empty()) d.transforms.push_back(identity_transform());
  if (d.materials.empty()) d.materials.push_back(default_material());
  if (d.textures.empty()) d.textures.push_back(default_texture());
  for (auto& t : d.textures) t.info.pixels = t.level0.data();
  if (!hip_ok(hipSetDevice(inst->device), "hipSetDevice", err)) return nullptr;
  if (!valid_references(d, err)) return nullptr;
  Composed at_exit{*s};
  if (!s->upload_geometry(err)) return nullptr;
  if (!s->textures_.upload(inst->stream, d.textures, err)) return nullptr;
  if (!s->tables_.build_materials(inst->stream, d.materials, err)) return nullptr;
  if (!s->tables_.build_lights_and_sky(inst->stream, d, s->geometry_.h_instances.size(), err)) return nullptr;
  if (!s->accel_.build(inst->build_options(), s->sources(), err)) return nullptr;
  if (!hip_ok(hipStreamSynchronize(inst->stream), "scene upload", err)) return nullptr;
  s->info.n_vertices = d.vertices.size();
  s->info.n_triangles = d.indices.size() / 3;
  s->info.n_instances = (uint32_t)s->geometry_.h_instances.size();
  s->info.n_materials = (uint32_t)d.materials.size();
  s->info.n_lights = s->tables_.lights_no;
  s->info.n_rt_lights = (uint32_t)s->tables_.h_lights.size();
  s->info.n_textures = (uint32_t)d.textures.size();
  return s.release();   // (at_exit goes first and holds the scene itself: the one that leaves is composed)
}

bool Scene::upload_geometry(Error& err) {
  hipStream_t st = instance->stream;
  SceneData& d = data;
  Geometry& g = geometry_;
  static_assert(sizeof(glz_vertex) == 2 * sizeof(float4), "vertex = 2 x float4");
  if (!hip_ok(g.vertices.upload(reinterpret_cast<const float4*>(d.vertices.data()), d.vertices.size() * 2, st), "upload vertices", err)) return false;
  if (!hip_ok(g.indices.upload(d.indices.data(), d.indices.size(), st), "upload indices", err)) return false;
  g.h_instances = rt_instances(d);
  if (!hip_ok(g.instances.upload(g.h_instances.data(), g.h_instances.size(), st), "upload instances", err)) return false;
  g.h_inst_base.assign(g.h_instances.size(), 0);
  uint64_t total = 0;
  for (size_t i = 0; i < g.h_instances.size(); ++i) {
    g.h_inst_base[i] = (uint32_t)total;
    total += g.h_instances[i].index_count / 3;
  }
  if (total >= 0x7FFFFFFFull) return err.fail(GLZ_E_UNSUPPORTED, "more than 2^31 world triangles");
  g.n_world_triangles = info.n_world_triangles = total;
  if (!hip_ok(g.inst_base.upload(g.h_inst_base.data(), g.h_inst_base.size(), st), "upload instance bases", err)) return false;
  // transforms + inverses (gl_WorldToObjectEXT is supplied by the driver in the reference)
  const std::vector<TransformPair> xf = transform_pairs(d.transforms);
  if (!hip_ok(g.transforms.upload(xf.data(), xf.size(), st), "upload transforms", err)) return false;
  float lut[256];
  for (int i = 0; i < 256; ++i) {   // sRGB EOTF of the R8G8B8A8_SRGB format (scene.rs:1028-1032) [ext]
    const double c = i / 255.0;
    lut[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
  }
  if (!hip_ok(g.srgb_lut.upload(lut, 256, st), "upload sRGB LUT", err)) return false;
  // calculate_geometric_derivatives (scene.rs:2113-2188)
  uint32_t ntri = 0;
  for (const glz_mesh& m : d.meshes) ntri = std::max<uint32_t>(ntri, (m.index_offset + m.index_count) / 3);
  if (!hip_ok(g.derivatives.alloc((size_t)ntri * 3), "alloc derivatives", err)) return false;
  if (!hip_ok(launch_derivatives(st, g.vertices.ptr, g.indices.ptr, ntri, g.derivatives.ptr), "derivatives kernel", err)) return false;
  // the host staging vectors above must outlive the async copies
  return hip_ok(hipStreamSynchronize(st), "geometry upload", err);
}

bool Scene::ensure_mips(Error& err) {
  if (textures_.mips_ready()) return true;
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  Composed at_exit{*this};
  return textures_.ensure_mips(instance->stream, data.textures, err);
}

bool Scene::read_mip_level(uint32_t texture, uint32_t level, std::vector<uint8_t>& pixels, uint32_t& w, uint32_t& h, Error& err) {
  pixels.clear();
  w = h = 0;
  if (texture >= data.textures.size()) return true;
  const TextureData& t = data.textures[texture];
  if (level == 0) {
    pixels = t.level0;
    w = t.info.width;
    h = t.info.height;
    return true;
  }
  if (!ensure_mips(err)) return false;
  const std::vector<uint8_t>* px = textures_.mip_level(texture, level);
  if (!px) return true;
  pixels = *px;
  w = host::mip_dim(t.info.width, level);
  h = host::mip_dim(t.info.height, level);
  return true;
}

bool Scene::update_materials_and_lights(const glz_material* mats, uint32_t n_mats, const glz_light* lights, uint32_t n_lights,
                                        const glz_texture* textures, uint32_t n_textures, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  if (n_mats != data.materials.size())
    return err.fail(GLZ_E_ARG, "update_materials_and_lights: the material count must not change (meshes index materials)");
  const size_t nt = textures ? n_textures : data.textures.size();
  for (uint32_t i = 0; i < n_mats; ++i) {
    const glz_material& m = mats[i];
    if (m.diffuse >= nt || m.roughness >= nt || m.metalness >= nt || m.normal >= nt || m.opacity >= nt)
      return err.fail(GLZ_E_INVALID_DATA, "material references a missing texture");
  }
  for (uint32_t i = 0; i < n_lights; ++i)
    if (lights[i].ltype == GLZ_LIGHT_SKY && lights[i].resource_id >= nt) return err.fail(GLZ_E_INVALID_DATA, "sky light references a missing texture");
  if (!mirror_for_accel(err)) return false;
  hipStream_t st = instance->stream;
  Composed at_exit{*this};
  if (textures) {
    if (!Textures::copy_of(textures, n_textures, data.textures, err) || !textures_.upload(st, data.textures, err)) return false;
    info.n_textures = n_textures;
    tables_.forget_sky_distribution();   // the sky map's texels may have changed: its distributions are rebuilt
  }
  bool opacity_changed = false;
  for (uint32_t i = 0; i < n_mats; ++i) opacity_changed |= (mats[i].opacity != 0) != (data.materials[i].opacity != 0);
  data.materials.assign(mats, mats + n_mats);
  data.lights.assign(lights, lights + n_lights);
  if (!tables_.build_materials(st, data.materials, err)) return false;
  if (!tables_.build_lights_and_sky(st, data, geometry_.h_instances.size(), err)) return false;
  // the non-opaque flag lives in the leaf records: the structure again, as the instance says now (the shape may change)
  if (opacity_changed && !accel_.build(instance->build_options(), sources(), err)) return false;
  if (!accel_.build_alpha_records(sources(), err)) return false;   // which opacity map a material names, where its texels lie
  info.n_lights = tables_.lights_no;
  info.n_rt_lights = (uint32_t)tables_.h_lights.size();
  return hip_ok(hipStreamSynchronize(st), "update_materials_and_lights", err);
}

bool Scene::debug_set_spectra(uint32_t material, const float* ior, const float* ior2abs2, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  Composed at_exit{*this};
  return tables_.debug_set_spectra(instance->stream, material, ior, ior2abs2, err);
}

// refresh_binded_textures (raytracer.rs:328-356): the texture array changed under the same materials and lights
bool Scene::refresh_textures(const glz_texture* textures, uint32_t n, Error& err) {
  const size_t nm = data.materials.size();
  std::vector<glz_material> mats = data.materials;
  std::vector<glz_light> lights = data.lights;
  return update_materials_and_lights(mats.data(), (uint32_t)nm, lights.data(), (uint32_t)lights.size(), textures, n, err);
}

bool Scene::instance_boxes(bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err) {
  if (!mirror_for_accel(err)) {
    lo.clear();
    hi.clear();
    return false;
  }
  if (!on_device || !accel_.two_level()) return accel_.instance_boxes(sources(), false, budget, lo, hi, err);
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) {
    lo.clear();
    hi.clear();
    return false;
  }
  Composed at_exit{*this};
  return accel_.instance_boxes(sources(), true, budget, lo, hi, err);
}

bool Scene::update_transforms(const glz_transform* transforms, uint32_t n, Error& err) {
  if (!transforms || n != data.transforms.size())
    return err.fail(GLZ_E_ARG, "update_transforms: the transform count must not change (instances index transforms)");
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err) || !mirror_for_accel(err)) return false;
  data.transforms.assign(transforms, transforms + n);
  const std::vector<TransformPair> xf = transform_pairs(data.transforms);
  if (!hip_ok(hipMemcpyAsync(geometry_.transforms.ptr, xf.data(), sizeof(TransformPair) * n, hipMemcpyHostToDevice, instance->stream), "upload transforms", err) ||
      !hip_ok(hipStreamSynchronize(instance->stream), "upload transforms", err))
    return false;
  Composed at_exit{*this};
  return accel_.rebuild(sources(), err);
}

bool Scene::geometry_update_info(glz_geometry_update_info& out, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  Composed at_exit{*this};
  return accel_.geometry_update(sources(), out, err);
}

bool Scene::update_vertices(const glz_vertex* vertices, uint32_t first, uint32_t n, int mode, Error& err) {
  if (!vertices || n == 0 || (uint64_t)first + n > data.vertices.size())
    return err.fail(GLZ_E_ARG, "update_vertices: null vertices, none, or a range past the scene's vertex count");
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return err.fail(GLZ_E_ARG, "update_vertices: unknown mode");
  // (valid_geometry, which creation runs, looks at index ranges and references alone: no position is refused there, so none is here)
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  if (!mirror_for_accel(err)) return false;   // (before the new ones go into it: a span read back later would be the device's all the same)
  hipStream_t st = instance->stream;
  Composed at_exit{*this};
  if (mode == GLZ_GEOMETRY_REFIT && !accel_.prepare_refit(sources(), err)) return false;   // needs the vertices the structure was built from
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  std::copy(vertices, vertices + n, data.vertices.begin() + first);
  if (!hip_ok(hipMemcpyAsync(geometry_.vertices.ptr + 2 * (size_t)first, data.vertices.data() + first, sizeof(glz_vertex) * n, hipMemcpyHostToDevice, st), "upload vertices", err))
    return false;
  // the normal sets the new positions reach: their normals are the device's to make (the mirror's positions stay current: the instance
  // boxes of a two-level scene read nothing else of it)
  if (!run_normals(first, n, st, err)) return false;
  if (!hip_ok(launch_derivatives(st, geometry_.vertices.ptr, geometry_.indices.ptr, (uint32_t)(geometry_.derivatives.count / 3), geometry_.derivatives.ptr), "derivatives kernel", err))
    return false;
  return accel_.update_geometry(sources(), mode, first, n, timer, err);
}

// ---- skinned meshes ----

const SceneData* Scene::host_data(Error& err) {
  if (stale_count_ == 0) return &data;
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err) ||
      !hip_ok(hipMemcpyAsync(data.vertices.data() + stale_first_, geometry_.vertices.ptr + 2 * (size_t)stale_first_, sizeof(glz_vertex) * stale_count_, hipMemcpyDeviceToHost,
                             instance->stream), "read posed vertices", err) ||
      !hip_ok(hipStreamSynchronize(instance->stream), "read posed vertices", err))
    return nullptr;
  stale_count_ = 0;
  return &data;
}

bool Scene::read_vertices(uint32_t first, uint32_t n, glz_vertex* out, Error& err) {
  if (!out || n == 0 || (uint64_t)first + n > data.vertices.size())
    return err.fail(GLZ_E_ARG, "read_vertices: null output, none, or a range past the scene's vertex count");
  return hip_ok(hipSetDevice(instance->device), "hipSetDevice", err) &&
         hip_ok(hipMemcpyAsync(out, geometry_.vertices.ptr + 2 * (size_t)first, sizeof(glz_vertex) * n, hipMemcpyDeviceToHost, instance->stream), "read vertices", err) &&
         hip_ok(hipStreamSynchronize(instance->stream), "read vertices", err);
}

// the device half of add_skin and copy_skins: every buffer of the skin, or none of it
int Scene::install_skin(int id, uint32_t first, std::vector<glz_vertex>&& bind, std::vector<uint16_t>&& joints, std::vector<float>&& weights, uint32_t n_bones,
                        int blend, const float4* device_bind, Error& err) {
  hipStream_t st = instance->stream;
  Skin s;
  s.first = first;
  s.n = (uint32_t)bind.size();
  s.n_bones = n_bones;
  s.blend = blend;
  s.h_bind = std::move(bind);
  s.h_joints = std::move(joints);
  s.h_weights = std::move(weights);
  static_assert(sizeof(uint2) == 4 * sizeof(uint16_t) && sizeof(glz_vertex) == 2 * sizeof(float4), "four joints are one uint2, a vertex two float4");
  // the bind pose: device to device from the scene's own vertices (add_skin), or from the host copy (a replica on another device)
  hipError_t bound = device_bind ? s.bind.alloc(2 * (size_t)s.n) : s.bind.upload(reinterpret_cast<const float4*>(s.h_bind.data()), 2 * (size_t)s.n, st);
  if (bound == hipSuccess && device_bind) bound = hipMemcpyAsync(s.bind.ptr, device_bind, sizeof(float4) * 2 * (size_t)s.n, hipMemcpyDeviceToDevice, st);
  if (!hip_ok(bound, "bind pose", err) ||
      !hip_ok(s.joints.upload(reinterpret_cast<const uint2*>(s.h_joints.data()), s.n, st), "upload joints", err) ||
      !hip_ok(s.weights.upload(reinterpret_cast<const float4*>(s.h_weights.data()), s.n, st), "upload weights", err) ||
      !hip_ok(hipStreamSynchronize(st), "add_skin", err))
    return -1;
  skins_.emplace(id, std::move(s));
  return id;
}

int Scene::add_skin(const glz_skin& k, Error& err) {
  auto refuse = [&](const char* why) {
    err.fail(GLZ_E_ARG, why);
    return -1;
  };
  if (!k.joints || !k.weights) return refuse("add_skin: joints or weights is null");
  if (k.n_vertices == 0 || (uint64_t)k.first_vertex + k.n_vertices > data.vertices.size()) return refuse("add_skin: no vertices, or a range past the scene's vertex count");
  if (k.n_bones == 0 || k.n_bones > 65536u) return refuse("add_skin: n_bones must be 1 .. 65536 (joints are 16 bits)");
  for (size_t i = 0; i < 4 * (size_t)k.n_vertices; ++i)
    if (k.joints[i] >= k.n_bones) return refuse("add_skin: a joint names a bone past n_bones");
  for (const auto& kv : skins_)
    if (k.first_vertex < (uint64_t)kv.second.first + kv.second.n && kv.second.first < (uint64_t)k.first_vertex + k.n_vertices)
      return refuse("add_skin: the range overlaps an existing skin");
  for (const auto& kv : morphs_)
    if (kv.second.skin < 0 && k.first_vertex < (uint64_t)kv.second.first + kv.second.n && kv.second.first < (uint64_t)k.first_vertex + k.n_vertices)
      return refuse("add_skin: the range overlaps a free-standing morph");
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return -1;
  // the bind pose is what the device holds now (the mirror may be behind it); the host copy of it is for replicas made later
  std::vector<glz_vertex> bind(k.n_vertices);
  if (!read_vertices(k.first_vertex, k.n_vertices, bind.data(), err)) return -1;
  const int id = install_skin(next_skin_, k.first_vertex, std::move(bind), std::vector<uint16_t>(k.joints, k.joints + 4 * (size_t)k.n_vertices),
                              std::vector<float>(k.weights, k.weights + 4 * (size_t)k.n_vertices), k.n_bones, GLZ_SKIN_LINEAR,
                              geometry_.vertices.ptr + 2 * (size_t)k.first_vertex, err);
  if (id >= 0) ++next_skin_;
  return id;
}

bool Scene::remove_skin(int id, Error& err) {
  const auto it = skins_.find(id);
  if (it == skins_.end()) return err.fail(GLZ_E_ARG, "remove_skin: no such skin");
  if (it->second.morph >= 0) return err.fail(GLZ_E_ARG, "remove_skin: the skin still carries a morph (remove_morph first)");
  skins_.erase(it);
  return true;
}

bool Scene::set_skin_blend(int id, int blend, Error& err) {
  const auto it = skins_.find(id);
  if (it == skins_.end()) return err.fail(GLZ_E_ARG, "set_skin_blend: no such skin");
  if (blend != GLZ_SKIN_LINEAR && blend != GLZ_SKIN_DUAL_QUATERNION) return err.fail(GLZ_E_ARG, "set_skin_blend: unknown blend mode");
  it->second.blend = blend;   // no bones are kept between calls: the next pose packs its bones for this mode
  return true;
}

int Scene::skin_blend(int id, Error& err) const {
  const auto it = skins_.find(id);
  if (it == skins_.end()) {
    err.fail(GLZ_E_ARG, "skin_blend: no such skin");
    return -1;
  }
  return it->second.blend;
}

bool Scene::copy_skins(const Scene& src, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  for (const auto& kv : src.skins_) {
    const Skin& s = kv.second;
    if (install_skin(kv.first, s.first, std::vector<glz_vertex>(s.h_bind), std::vector<uint16_t>(s.h_joints), std::vector<float>(s.h_weights), s.n_bones, s.blend, nullptr, err) < 0)
      return false;
  }
  next_skin_ = src.next_skin_;
  return true;
}

bool Scene::posed_span(const glz_pose* poses, uint32_t n_poses, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string(who) + ": " + why); };
  if (!poses || n_poses == 0) return refuse("poses is null or empty");
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = 0; i < n_poses; ++i) {
    const auto it = skins_.find(poses[i].skin);
    if (it == skins_.end()) return refuse("no such skin");
    if (!poses[i].bones) return refuse("a pose's bones are null");
    if (poses[i].n_bones != it->second.n_bones) return refuse("a pose's bone count is not its skin's");
    for (uint32_t k = 0; k < i; ++k)
      if (poses[k].skin == poses[i].skin) return refuse("a skin is named twice");
    lo = std::min<uint64_t>(lo, it->second.first);
    hi = std::max<uint64_t>(hi, (uint64_t)it->second.first + it->second.n);
  }
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  return true;
}

bool Scene::upload_bones(const glz_pose& pose, std::vector<float4>& packed, DeviceBuffer<float4>& bones, hipStream_t st, Error& err) const {
  const Skin& s = skins_.at(pose.skin);
  const uint32_t rows = post::bone_rows(s.blend);
  packed.resize((size_t)rows * s.n_bones);
  for (uint32_t b = 0; b < s.n_bones; ++b) {
    if (s.blend == GLZ_SKIN_DUAL_QUATERNION) post::pack_bone_dq(pose.bones[b], packed.data() + (size_t)rows * b);
    else post::pack_bone(pose.bones[b], packed.data() + (size_t)rows * b);
  }
  if (bones.ptr == nullptr || bones.count != packed.size()) {
    if (!hip_ok(bones.alloc(packed.size()), "alloc bones", err)) return false;
  }
  return hip_ok(hipMemcpyAsync(bones.ptr, packed.data(), sizeof(float4) * packed.size(), hipMemcpyHostToDevice, st), "upload bones", err);
}

bool Scene::skin_into(const glz_pose& pose, float4* span, uint32_t span_first, std::vector<float4>& packed, DeviceBuffer<float4>& bones, hipStream_t st, Error& err) const {
  const Skin& s = skins_.at(pose.skin);
  const auto launch = s.blend == GLZ_SKIN_DUAL_QUATERNION ? launch_skin_dq : launch_skin;
  return upload_bones(pose, packed, bones, st, err) &&
         hip_ok(launch(st, s.bind.ptr, s.joints.ptr, s.weights.ptr, s.n, bones.ptr, s.n_bones, span + 2 * (size_t)(s.first - span_first)),
                s.blend == GLZ_SKIN_DUAL_QUATERNION ? "k_skin_dq" : "k_skin", err);
}

bool Scene::time_skin(const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const {
  uint32_t first = 0, count = 0;
  if (!kernel_ms || reps == 0) return err.fail(GLZ_E_ARG, "skin timing: null output or no repeats");
  if (!posed_span(&pose, 1, "skin timing", first, count, err)) return false;
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  hipStream_t st = instance->stream;
  std::vector<float4> packed;
  DeviceBuffer<float4> bones, out;
  Events<2> t;
  if (!hip_ok(out.alloc(2 * (size_t)count), "alloc", err) || !t.create(err) || !skin_into(pose, out.ptr, first, packed, bones, st, err)) return false;
  (void)hipEventRecord(t.ev[0], st);
  for (uint32_t i = 0; i < reps; ++i)
    if (!skin_into(pose, out.ptr, first, packed, bones, st, err)) return false;
  (void)hipEventRecord(t.ev[1], st);
  if (!hip_ok(hipStreamSynchronize(st), "skin timing", err)) return false;
  (void)hipEventElapsedTime(kernel_ms, t.ev[0], t.ev[1]);
  *kernel_ms /= (float)reps;
  return true;
}

bool Scene::pose_skins(const glz_pose* poses, uint32_t n_poses, int mode, Error& err) {
  return run_animation(glz_animation{nullptr, 0, poses, n_poses}, mode, "pose_skins", err);
}

// ---- morph targets ----

int Scene::install_morph(int id, uint32_t first, int skin, std::vector<glz_vertex>&& base, post::MorphLayout&& layout, const float4* device_base, Error& err) {
  hipStream_t st = instance->stream;
  Morph m;
  m.first = first;
  m.n = layout.n_vertices;
  m.n_targets = layout.n_targets;
  m.n_entries = layout.n_entries;
  m.skin = skin;
  m.h_base = std::move(base);
  m.layout = std::move(layout);
  hipError_t based = hipSuccess;
  if (skin < 0) {   // its own base: device to device from the scene's vertices (add_morph), or from the host copy (a replica on another device)
    based = device_base ? m.base.alloc(2 * (size_t)m.n) : m.base.upload(reinterpret_cast<const float4*>(m.h_base.data()), 2 * (size_t)m.n, st);
    if (based == hipSuccess && device_base) based = hipMemcpyAsync(m.base.ptr, device_base, sizeof(float4) * 2 * (size_t)m.n, hipMemcpyDeviceToDevice, st);
  }
  if (!hip_ok(based, "morph base", err) || !hip_ok(m.counts.upload(m.layout.counts.data(), m.layout.counts.size(), st), "upload morph counts", err) ||
      !hip_ok(m.slices.upload(m.layout.slices.data(), m.layout.slices.size(), st), "upload morph slices", err) ||
      !hip_ok(m.entries.upload(m.layout.entries.data(), m.layout.entries.size(), st), "upload morph entries", err) || !hip_ok(hipStreamSynchronize(st), "add_morph", err))
    return -1;
  if (skin >= 0) skins_.at(skin).morph = id;
  morphs_.emplace(id, std::move(m));
  return id;
}

int Scene::add_morph(const glz_morph& g, Error& err) {
  auto refuse = [&](const std::string& why) {
    err.fail(GLZ_E_ARG, "add_morph: " + why);
    return -1;
  };
  if (g.n_vertices == 0 || (uint64_t)g.first_vertex + g.n_vertices > data.vertices.size()) return refuse("no vertices, or a range past the scene's vertex count");
  const uint64_t lo = g.first_vertex, hi = lo + g.n_vertices;
  if (g.skin >= 0) {
    const auto it = skins_.find(g.skin);
    if (it == skins_.end()) return refuse("no such skin");
    if (it->second.morph >= 0) return refuse("the skin already carries a morph");
    if (it->second.first != g.first_vertex || it->second.n != g.n_vertices) return refuse("an attached morph's range must be exactly its skin's");
  } else {
    if (g.skin != -1) return refuse("skin must be a skin's id, or -1");
    for (const auto& kv : skins_)
      if (lo < (uint64_t)kv.second.first + kv.second.n && kv.second.first < hi) return refuse("the range overlaps a skin");
    for (const auto& kv : morphs_)
      if (lo < (uint64_t)kv.second.first + kv.second.n && kv.second.first < hi) return refuse("the range overlaps an existing morph");
  }
  post::MorphLayout layout;
  std::string why;
  if (!post::pack_morph(g.n_vertices, g.targets, g.n_targets, layout, why)) return refuse(why);
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return -1;
  std::vector<glz_vertex> base;
  if (g.skin < 0) {   // the base is what the device holds now; the host copy of it is for replicas made later
    base.resize(g.n_vertices);
    if (!read_vertices(g.first_vertex, g.n_vertices, base.data(), err)) return -1;
  }
  const int id = install_morph(next_morph_, g.first_vertex, g.skin, std::move(base), std::move(layout), geometry_.vertices.ptr + 2 * (size_t)g.first_vertex, err);
  if (id >= 0) ++next_morph_;
  return id;
}

bool Scene::remove_morph(int id, Error& err) {
  const auto it = morphs_.find(id);
  if (it == morphs_.end()) return err.fail(GLZ_E_ARG, "remove_morph: no such morph");
  if (it->second.skin >= 0) skins_.at(it->second.skin).morph = -1;
  morphs_.erase(it);
  return true;
}

bool Scene::copy_morphs(const Scene& src, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  for (const auto& kv : src.morphs_) {
    const Morph& m = kv.second;
    if (install_morph(kv.first, m.first, m.skin, std::vector<glz_vertex>(m.h_base), post::MorphLayout(m.layout), nullptr, err) < 0) return false;
  }
  next_morph_ = src.next_morph_;
  return true;
}

bool Scene::animated_span(const glz_animation* anim, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string(who) + ": " + why); };
  if (!anim) return refuse("the animation is null");
  if (anim->n_morphs == 0) return posed_span(anim->poses, anim->n_poses, who, first, count, err);
  if (!anim->morphs) return refuse("morphs is null");
  uint64_t lo = ~0ull, hi = 0;
  if (anim->n_poses) {
    if (!posed_span(anim->poses, anim->n_poses, who, first, count, err)) return false;
    lo = first;
    hi = (uint64_t)first + count;
  }
  for (uint32_t i = 0; i < anim->n_morphs; ++i) {
    const glz_morph_weights& w = anim->morphs[i];
    const auto it = morphs_.find(w.morph);
    if (it == morphs_.end()) return refuse("no such morph");
    if (!w.weights) return refuse("a morph's weights are null");
    if (w.n_targets != it->second.n_targets) return refuse("a morph's target count is not its morph's");
    for (uint32_t k = 0; k < i; ++k)
      if (anim->morphs[k].morph == w.morph) return refuse("a morph is named twice");
    if (it->second.skin >= 0) {   // no bones are kept between calls: the skin's pose must come with it
      bool posed = false;
      for (uint32_t k = 0; k < anim->n_poses; ++k) posed = posed || anim->poses[k].skin == it->second.skin;
      if (!posed) return refuse("an attached morph is named without its skin's pose");
    }
    lo = std::min<uint64_t>(lo, it->second.first);
    hi = std::max<uint64_t>(hi, (uint64_t)it->second.first + it->second.n);
  }
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  return true;
}

MorphArgs Scene::morph_args(const Morph& m, const float* weights) const {
  return MorphArgs{m.skin >= 0 ? skins_.at(m.skin).bind.ptr : m.base.ptr, m.counts.ptr, m.slices.ptr, m.entries.ptr, m.n, weights, m.n_targets};
}

static bool upload_morph_weights(const glz_morph_weights& w, DeviceBuffer<float>& buffer, hipStream_t st, Error& err) {
  if (buffer.ptr == nullptr || buffer.count != w.n_targets) {
    if (!hip_ok(buffer.alloc(w.n_targets), "alloc morph weights", err)) return false;
  }
  return hip_ok(hipMemcpyAsync(buffer.ptr, w.weights, sizeof(float) * w.n_targets, hipMemcpyHostToDevice, st), "upload morph weights", err);
}

bool Scene::animate_into(const glz_animation& anim, float4* span, uint32_t span_first, AnimationUploads& up, hipStream_t st, Error& err) const {
  up.packed.resize(anim.n_poses);
  up.bones.resize(anim.n_poses);
  up.weights.resize(anim.n_morphs);
  for (uint32_t i = 0; i < anim.n_morphs; ++i) {
    const Morph& m = morphs_.at(anim.morphs[i].morph);
    if (!upload_morph_weights(anim.morphs[i], up.weights[i], st, err)) return false;
    if (m.skin < 0 && !hip_ok(launch_morph(st, morph_args(m, up.weights[i].ptr), span + 2 * (size_t)(m.first - span_first)), "k_morph", err)) return false;
  }
  for (uint32_t i = 0; i < anim.n_poses; ++i) {
    const glz_pose& pose = anim.poses[i];
    const Skin& s = skins_.at(pose.skin);
    uint32_t named = anim.n_morphs;   // where the skin's morph is named, if it is
    for (uint32_t k = 0; k < anim.n_morphs && s.morph >= 0; ++k)
      if (anim.morphs[k].morph == s.morph) named = k;
    if (named == anim.n_morphs) {
      if (!skin_into(pose, span, span_first, up.packed[i], up.bones[i], st, err)) return false;
      continue;
    }
    const auto launch = s.blend == GLZ_SKIN_DUAL_QUATERNION ? launch_morph_skin_dq : launch_morph_skin;
    if (!upload_bones(pose, up.packed[i], up.bones[i], st, err) ||
        !hip_ok(launch(st, morph_args(morphs_.at(s.morph), up.weights[named].ptr), s.joints.ptr, s.weights.ptr, up.bones[i].ptr, s.n_bones,
                       span + 2 * (size_t)(s.first - span_first)), s.blend == GLZ_SKIN_DUAL_QUATERNION ? "k_morph_skin_dq" : "k_morph_skin", err))
      return false;
  }
  return true;
}

bool Scene::time_morph(const glz_animation& one, uint32_t reps, float* kernel_ms, uint64_t* bytes, Error& err) const {
  auto refuse = [&](const char* why) { return err.fail(GLZ_E_ARG, std::string("morph timing: ") + why); };
  if (!kernel_ms || reps == 0) return refuse("null output or no repeats");
  if (!one.morphs || one.n_morphs != 1 || one.n_poses > 1) return refuse("one morph, alone or with its skin's pose");
  const bool fused = one.n_poses == 1;
  const glz_morph_weights& w = one.morphs[0];
  uint32_t first = 0, count = 0;
  if (fused && !animated_span(&one, "morph timing", first, count, err)) return false;
  const auto it = morphs_.find(w.morph);
  if (it == morphs_.end() || !w.weights || w.n_targets != it->second.n_targets) return refuse("no such morph, null weights, or a target count that is not the morph's");
  const Morph& m = it->second;
  if (fused && m.skin != one.poses[0].skin) return refuse("the pose is not of the morph's skin");
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  hipStream_t st = instance->stream;
  std::vector<float4> packed;
  DeviceBuffer<float4> bones, out;
  DeviceBuffer<float> weights;
  Events<2> t;
  if (!hip_ok(out.alloc(2 * (size_t)m.n), "alloc", err) || !t.create(err)) return false;
  auto once = [&] {
    if (!upload_morph_weights(w, weights, st, err)) return false;
    if (!fused) return hip_ok(launch_morph(st, morph_args(m, weights.ptr), out.ptr), "k_morph", err);
    const Skin& s = skins_.at(m.skin);
    const auto launch = s.blend == GLZ_SKIN_DUAL_QUATERNION ? launch_morph_skin_dq : launch_morph_skin;
    return upload_bones(one.poses[0], packed, bones, st, err) &&
           hip_ok(launch(st, morph_args(m, weights.ptr), s.joints.ptr, s.weights.ptr, bones.ptr, s.n_bones, out.ptr),
                  s.blend == GLZ_SKIN_DUAL_QUATERNION ? "k_morph_skin_dq" : "k_morph_skin", err);
  };
  if (!once()) return false;
  (void)hipEventRecord(t.ev[0], st);
  for (uint32_t i = 0; i < reps; ++i)
    if (!once()) return false;
  (void)hipEventRecord(t.ev[1], st);
  if (!hip_ok(hipStreamSynchronize(st), "morph timing", err)) return false;
  (void)hipEventElapsedTime(kernel_ms, t.ev[0], t.ev[1]);
  *kernel_ms /= (float)reps;
  if (bytes) {
    *bytes = (uint64_t)m.n * (32 + 32 + 4) + (uint64_t)m.layout.slices.size() * 8 + m.n_entries * 32 + (uint64_t)m.n_targets * 4;
    if (fused) *bytes += (uint64_t)m.n * (8 + 16) + (uint64_t)skins_.at(m.skin).n_bones * sizeof(float4) * post::bone_rows(skins_.at(m.skin).blend);
  }
  return true;
}

// ---- vertex normals from deformed positions ----

void Scene::mark_stale(uint32_t first, uint32_t count) {
  const uint64_t lo = stale_count_ ? std::min(stale_first_, first) : first;
  const uint64_t hi = stale_count_ ? std::max<uint64_t>((uint64_t)stale_first_ + stale_count_, (uint64_t)first + count) : (uint64_t)first + count;
  stale_first_ = (uint32_t)lo;
  stale_count_ = (uint32_t)(hi - lo);
}

NormalArgs Scene::normal_args(const NormalSet& s) {
  return NormalArgs{s.faces.ptr, s.layout.n_faces, s.counts.ptr, s.slices.ptr, s.rows.ptr, s.layout.n_vertices};
}

// the device half of add_normals and copy_normals: every buffer of the set, or none of it
int Scene::install_normals(int id, post::NormalLayout&& layout, Error& err) {
  hipStream_t st = instance->stream;
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

int Scene::add_normals(const glz_normals& g, Error& err) {
  auto refuse = [&](const std::string& why) {
    err.fail(GLZ_E_ARG, "add_normals: " + why);
    return -1;
  };
  if (g.n_vertices == 0 || (uint64_t)g.first_vertex + g.n_vertices > data.vertices.size()) return refuse("no vertices, or a range past the scene's vertex count");
  for (const auto& kv : normals_)
    if (g.first_vertex < (uint64_t)kv.second.layout.first + kv.second.layout.n_vertices && kv.second.layout.first < (uint64_t)g.first_vertex + g.n_vertices)
      return refuse("the range overlaps an existing normal set");
  post::NormalLayout layout;
  std::string why;
  if (!post::pack_normals(data.indices.data(), data.indices.size(), data.meshes.data(), data.meshes.size(), data.vertices.size(), g.first_vertex, g.n_vertices, g.groups,
                          layout, why))
    return refuse(why);
  // from here on it is update_vertices(REFIT) over the set's range, with the two kernels where the upload is
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err) || !mirror_for_accel(err)) return -1;
  hipStream_t st = instance->stream;
  Composed at_exit{*this};
  if (!accel_.prepare_refit(sources(), err)) return -1;
  StreamTimer timer;
  if (!timer.start(st, err)) return -1;
  const int id = install_normals(next_normals_, std::move(layout), err);
  if (id < 0) return -1;
  ++next_normals_;
  const NormalSet& s = normals_.at(id);
  mark_stale(g.first_vertex, g.n_vertices);
  float4* range = geometry_.vertices.ptr + 2 * (size_t)g.first_vertex;
  if (!hip_ok(launch_face_vectors(st, geometry_.vertices.ptr, normal_args(s), s.face_vectors.ptr), "k_face_vectors", err) ||
      !hip_ok(launch_vertex_normals(st, range, normal_args(s), s.face_vectors.ptr, range), "k_vertex_normals", err) ||
      !hip_ok(launch_derivatives(st, geometry_.vertices.ptr, geometry_.indices.ptr, (uint32_t)(geometry_.derivatives.count / 3), geometry_.derivatives.ptr), "derivatives kernel", err) ||
      !accel_.update_geometry(sources(), GLZ_GEOMETRY_REFIT, g.first_vertex, g.n_vertices, timer, err)) {   // (the mirror's positions are current)
    normals_.erase(id);
    return -1;
  }
  return id;
}

bool Scene::remove_normals(int id, Error& err) {
  if (normals_.erase(id) == 0) return err.fail(GLZ_E_ARG, "remove_normals: no such normal set");
  return true;
}

bool Scene::copy_normals(const Scene& src, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  for (const auto& kv : src.normals_)
    if (install_normals(kv.first, post::NormalLayout(kv.second.layout), err) < 0) return false;
  next_normals_ = src.next_normals_;
  return true;
}

bool Scene::run_normals(uint32_t& first, uint32_t& count, hipStream_t st, Error& err) {
  uint64_t lo = first, hi = (uint64_t)first + count;
  const uint64_t written_lo = lo, written_hi = hi;
  bool any = false;
  for (const auto& kv : normals_) {
    const NormalSet& s = kv.second;
    // (the rule is a function of positions alone: the whole set again, and what did not change comes out with the bits it had)
    if (s.layout.n_faces == 0 || s.layout.reach_lo >= written_hi || s.layout.reach_hi < written_lo) continue;
    float4* range = geometry_.vertices.ptr + 2 * (size_t)s.layout.first;
    if (!hip_ok(launch_face_vectors(st, geometry_.vertices.ptr, normal_args(s), s.face_vectors.ptr), "k_face_vectors", err) ||
        !hip_ok(launch_vertex_normals(st, range, normal_args(s), s.face_vectors.ptr, range), "k_vertex_normals", err))
      return false;
    lo = std::min<uint64_t>(lo, s.layout.first);
    hi = std::max<uint64_t>(hi, (uint64_t)s.layout.first + s.layout.n_vertices);
    any = true;
  }
  if (!any) return true;
  first = (uint32_t)lo;
  count = (uint32_t)(hi - lo);
  mark_stale(first, count);
  return true;
}

bool Scene::time_normals(int id, uint32_t reps, float ms[2], uint64_t bytes[2], Error& err) const {
  const auto it = normals_.find(id);
  if (!ms || reps == 0 || it == normals_.end()) return err.fail(GLZ_E_ARG, "normals timing: null output, no repeats, or no such normal set");
  const NormalSet& s = it->second;
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  hipStream_t st = instance->stream;
  DeviceBuffer<float4> face_vectors, out;
  Events<3> t;
  const float4* range = geometry_.vertices.ptr + 2 * (size_t)s.layout.first;
  if (!hip_ok(face_vectors.alloc(std::max<size_t>(s.layout.n_faces, 1)), "alloc", err) || !hip_ok(out.alloc(2 * (size_t)s.layout.n_vertices), "alloc", err) || !t.create(err) ||
      !hip_ok(hipMemcpyAsync(out.ptr, range, sizeof(float4) * 2 * (size_t)s.layout.n_vertices, hipMemcpyDeviceToDevice, st), "copy vertices", err))
    return false;
  auto faces = [&] { return hip_ok(launch_face_vectors(st, geometry_.vertices.ptr, normal_args(s), face_vectors.ptr), "k_face_vectors", err); };
  auto vertices = [&] { return hip_ok(launch_vertex_normals(st, range, normal_args(s), face_vectors.ptr, out.ptr), "k_vertex_normals", err); };
  if (!faces() || !vertices()) return false;
  (void)hipEventRecord(t.ev[0], st);
  for (uint32_t i = 0; i < reps; ++i)
    if (!faces()) return false;
  (void)hipEventRecord(t.ev[1], st);
  for (uint32_t i = 0; i < reps; ++i)
    if (!vertices()) return false;
  (void)hipEventRecord(t.ev[2], st);
  if (!hip_ok(hipStreamSynchronize(st), "normals timing", err)) return false;
  (void)hipEventElapsedTime(&ms[0], t.ev[0], t.ev[1]);
  (void)hipEventElapsedTime(&ms[1], t.ev[1], t.ev[2]);
  ms[0] /= (float)reps;
  ms[1] /= (float)reps;
  if (bytes) {
    uint64_t with_faces = 0;
    for (uint32_t c : s.layout.counts) with_faces += c != 0;
    bytes[0] = (uint64_t)s.layout.n_faces * (12 + 3 * 16 + 16);
    bytes[1] = (uint64_t)s.layout.n_vertices * 4 + (uint64_t)s.layout.slices.size() * 8 + s.layout.n_entries * (4 + 16) + with_faces * (32 + 12);
  }
  return true;
}

bool Scene::animate(const glz_animation& anim, int mode, Error& err) { return run_animation(anim, mode, "animate", err); }

bool Scene::run_animation(const glz_animation& anim, int mode, const char* who, Error& err) {
  uint32_t first = 0, count = 0;
  if (!animated_span(&anim, who, first, count, err)) return false;
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return err.fail(GLZ_E_ARG, std::string(who) + ": unknown mode");
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  hipStream_t st = instance->stream;
  Composed at_exit{*this};
  if (mode == GLZ_GEOMETRY_REFIT && !accel_.prepare_refit(sources(), err)) return false;   // needs the vertices the structure was built from
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  // whatever happens from here on, the device's vertices may differ from the mirror's over the span (joined with a span still pending)
  mark_stale(first, count);
  // (the uploads outlive the copies: update_geometry waits for the stream; the buffers are the scene's, reused while the calls name as much)
  if (!animate_into(anim, geometry_.vertices.ptr, 0, uploads_, st, err)) return false;
  if (!run_normals(first, count, st, err)) return false;   // the normal sets the written span reaches; the span grows by their ranges
  if (!hip_ok(launch_derivatives(st, geometry_.vertices.ptr, geometry_.indices.ptr, (uint32_t)(geometry_.derivatives.count / 3), geometry_.derivatives.ptr), "derivatives kernel", err))
    return false;
  if (!mirror_for_accel(err)) return false;   // two levels: the top level is rebuilt from the meshes' points
  return accel_.update_geometry(sources(), mode, first, count, timer, err);
}

}  // namespace glz
