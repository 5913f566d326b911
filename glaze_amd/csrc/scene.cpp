// RayTraceInstance::new / RayTraceScene::new on HIP (lib/src/vulkan/instance.rs:376-427,
// lib/src/vulkan/scene.rs:1414-1556 and the helpers it calls).
#include "scene.h"

#include <algorithm>
#include <cmath>

#include "host_math.h"
#include "mipchain.h"

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

template <class Write>
bool Scene::update_geometry(const char* who, int mode, bool mirror_first, const int& only, uint32_t first, uint32_t count, Write&& write, Error& err) {
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return err.fail(GLZ_E_ARG, std::string(who) + ": unknown mode");
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  if (mirror_first && !mirror_for_accel(err)) return false;
  hipStream_t st = instance->stream;
  Composed at_exit{*this};
  if (mode == GLZ_GEOMETRY_REFIT && !accel_.prepare_refit(sources(), err)) return false;   // needs the vertices the structure was built from
  StreamTimer timer;
  if (!timer.start(st, err) || !write(st)) return false;
  // the normal sets the written span reaches: their normals are the device's to make, and the span grows by their ranges
  bool ran = false;
  if (!deformers_.run_normals(deformer_sources(), only, first, count, ran, err)) return false;
  if (ran) mark_stale(first, count);
  if (!hip_ok(launch_derivatives(st, geometry_.vertices.ptr, geometry_.indices.ptr, (uint32_t)(geometry_.derivatives.count / 3), geometry_.derivatives.ptr), "derivatives kernel", err))
    return false;
  if (!mirror_first && !mirror_for_accel(err)) return false;   // two levels: the top level is rebuilt from the meshes' points
  return accel_.update_geometry(sources(), mode, first, count, timer, err);
}

bool Scene::update_vertices(const glz_vertex* vertices, uint32_t first, uint32_t n, int mode, Error& err) {
  if (!vertices || n == 0 || (uint64_t)first + n > data.vertices.size())
    return err.fail(GLZ_E_ARG, "update_vertices: null vertices, none, or a range past the scene's vertex count");
  // (valid_geometry, which creation runs, looks at index ranges and references alone: no position is refused there, so none is here)
  // The mirror is read back BEFORE the new vertices go into it (a span read back later would be the device's all the same), and not again
  // after the normal sets ran: its positions stay current, and the instance boxes of a two-level scene read nothing else of it.
  return update_geometry("update_vertices", mode, true, -1, first, n, [&](hipStream_t st) {
    std::copy(vertices, vertices + n, data.vertices.begin() + first);
    return hip_ok(hipMemcpyAsync(geometry_.vertices.ptr + 2 * (size_t)first, data.vertices.data() + first, sizeof(glz_vertex) * n, hipMemcpyHostToDevice, st), "upload vertices", err);
  }, err);
}

bool Scene::run_animation(const glz_animation& anim, int mode, const char* who, Error& err) {
  uint32_t first = 0, count = 0;
  if (!deformers_.animated_span(&anim, who, first, count, err)) return false;
  // The mirror comes up to date AFTER the derivatives (mirror_first = false), for two-level scenes only.
  return update_geometry(who, mode, false, -1, first, count, [&](hipStream_t) {
    // whatever happens from here on, the device's vertices may differ from the mirror's over the span (joined with a span still pending)
    mark_stale(first, count);
    // (the uploads outlive the copies: Accel::update_geometry waits for the stream)
    return deformers_.animate(deformer_sources(), anim, err);
  }, err);
}

bool Scene::play(const glz_play* plays, uint32_t n, int mode, Error& err) {
  uint32_t first = 0, count = 0;
  if (!deformers_.played_span(plays, n, "play", first, count, err)) return false;
  // as run_animation: the mirror comes up to date after the derivatives, and the span is stale from the first kernel on
  return update_geometry("play", mode, false, -1, first, count, [&](hipStream_t) {
    mark_stale(first, count);
    return deformers_.play(deformer_sources(), plays, n, err);   // (the table outlives its copy: Accel::update_geometry waits for the stream)
  }, err);
}

int Scene::add_normals(const glz_normals& g, Error& err) {
  post::NormalLayout layout;
  if (!deformers_.pack_normals(deformer_sources(), g, layout, err)) return -1;
  // from here on it is update_vertices(REFIT) over the set's range, with the set's two kernels where the upload is
  int id = -1;
  const bool done = update_geometry("add_normals", GLZ_GEOMETRY_REFIT, true, id, g.first_vertex, g.n_vertices, [&](hipStream_t) {
    id = deformers_.install_normals(deformer_sources(), std::move(layout), err);
    if (id >= 0) mark_stale(g.first_vertex, g.n_vertices);
    return id >= 0;
  }, err);   // (the mirror's positions are current)
  if (done) return id;
  Error rolled_back;   // whatever failed after the install: the set goes again
  if (id >= 0) deformers_.remove_normals(id, rolled_back);
  return -1;
}

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

void Scene::mark_stale(uint32_t first, uint32_t count) {
  const uint64_t lo = stale_count_ ? std::min(stale_first_, first) : first;
  const uint64_t hi = stale_count_ ? std::max<uint64_t>((uint64_t)stale_first_ + stale_count_, (uint64_t)first + count) : (uint64_t)first + count;
  stale_first_ = (uint32_t)lo;
  stale_count_ = (uint32_t)(hi - lo);
}

}  // namespace glz
