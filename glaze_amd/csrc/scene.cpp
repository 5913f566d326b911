// RayTraceInstance::new / RayTraceScene::new on HIP (lib/src/vulkan/instance.rs:376-427,
// lib/src/vulkan/scene.rs:1414-1556 and the helpers it calls).
#include "scene.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include <thread>

#include "host_math.h"
#include "kernels.h"
#include "mipchain.h"

namespace glz {

bool hip_ok(hipError_t e, const char* what, Error& err) {
  if (e == hipSuccess) return true;
  err.code = GLZ_E_DEVICE;
  err.msg = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

// Two HIP events around work on a stream, destroyed on every way out
struct StreamTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  StreamTimer() = default;
  StreamTimer(const StreamTimer&) = delete;
  StreamTimer& operator=(const StreamTimer&) = delete;
  ~StreamTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  bool start(hipStream_t st, Error& err) {
    if (!hip_ok(hipEventCreate(&e0), "event", err) || !hip_ok(hipEventCreate(&e1), "event", err)) return false;
    (void)hipEventRecord(e0, st);
    return true;
  }
  void stop(hipStream_t st) { (void)hipEventRecord(e1, st); }
  float ms() {   // waits for the stop event
    float v = 0.0f;
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&v, e0, e1);
    return v;
  }
};

Instance::~Instance() {
  if (stream) (void)hipStreamDestroy(stream);
}

Instance* Instance::create(int hip_device, Error& err) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    err.code = GLZ_E_DEVICE;
    err.msg = "no HIP device available";
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
      err.code = GLZ_E_ARG;
      err.msg = "HIP device ordinal out of range";
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
    err.code = GLZ_E_DEVICE;
    err.msg = "no gfx950 (MI355X) device found" + (arch.empty() ? std::string() : " (device is " + arch + ")");
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

// meshes are indexed by id, the last one with an id wins; null: no such mesh
static const glz_mesh* mesh_by_id(const SceneData& d, uint32_t id) {
  const glz_mesh* found = nullptr;
  for (const glz_mesh& m : d.meshes)
    if (m.id == id) found = &m;
  return found;
}

// load_raytrace_instances_to_gpu (scene.rs:1784-1818): dangling instances dropped
std::vector<RTInstance> rt_instances(const SceneData& d) {
  std::vector<RTInstance> out;
  for (const glz_mesh_instance& in : d.instances) {
    const glz_mesh* found = mesh_by_id(d, in.mesh_id);
    if (!found) continue;
    out.push_back(RTInstance{found->index_offset, found->index_count, found->material, in.transform_id});
  }
  return out;
}

// object -> world as given, world -> object inverted in double precision (identity when singular or not finite)
static std::vector<TransformPair> transform_pairs(const std::vector<glz_transform>& transforms) {
  std::vector<TransformPair> xf(transforms.size());
  for (size_t i = 0; i < xf.size(); ++i) {
    memcpy(xf[i].o2w, transforms[i].m, 64);
    host::Mat4d inv;
    if (!host::invert(host::Mat4d::from_f32(transforms[i].m), inv)) inv = host::Mat4d::identity();
    inv.to_f32(xf[i].w2o);
  }
  return xf;
}

// DeviceScene::xf_identity: 1 for a transform that is bitwise the identity (-0.0 does not count)
static std::vector<uint32_t> identity_flags(const std::vector<glz_transform>& transforms) {
  std::vector<uint32_t> ident(transforms.size(), 0u);
  for (size_t i = 0; i < ident.size(); ++i) {
    static const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    ident[i] = memcmp(transforms[i].m, id, 64) == 0 ? 1u : 0u;
  }
  return ident;
}

static uint32_t sbt_callable_index(uint8_t mtype) {   // materials/material.rs:244-258
  switch (mtype) {
    case GLZ_MAT_FLAT:
    case GLZ_MAT_LAMBERT: return kBsdfLambert;
    case GLZ_MAT_MIRROR: return kBsdfMirror;
    case GLZ_MAT_GLASS: return kBsdfGlass;
    case GLZ_MAT_METAL: return kBsdfMetal;
    case GLZ_MAT_FROSTED: return kBsdfFrosted;
    default: return kBsdfUber;
  }
}

// The distinct index ranges (offset, count) the instances draw, in first-use order (it fixes tri_base, node_base and the order in which
// the exact-box budget is spent), and which of them each instance uses.
static std::vector<std::pair<uint32_t, uint32_t>> unique_meshes(const std::vector<RTInstance>& instances, std::vector<uint32_t>& mesh_of) {
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  mesh_of.resize(instances.size());
  for (size_t i = 0; i < instances.size(); ++i) {
    const std::pair<uint32_t, uint32_t> key(instances[i].index_offset, instances[i].index_count);
    const size_t m = std::find(ranges.begin(), ranges.end(), key) - ranges.begin();
    if (m == ranges.size()) ranges.push_back(key);
    mesh_of[i] = (uint32_t)m;
  }
  return ranges;
}

// References inside the geometry, so that nothing indexes out of bounds: index ranges, vertex indices, transform ids
static bool valid_geometry(const SceneData& d, size_t n_transforms, Error& err) {
  auto fail = [&](const char* what) {
    err.code = GLZ_E_INVALID_DATA;
    err.msg = what;
    return false;
  };
  for (const glz_mesh& m : d.meshes)
    if ((uint64_t)m.index_offset + m.index_count > d.indices.size()) return fail("mesh index range outside the index buffer");
  for (uint32_t i : d.indices)
    if (i >= d.vertices.size()) return fail("vertex index out of range");
  for (const glz_mesh_instance& in : d.instances)
    if (in.transform_id >= n_transforms) return fail("instance references a missing transform");
  return true;
}

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
  // validate references so that no kernel can index out of bounds
  if (!valid_geometry(d, d.transforms.size(), err)) return nullptr;
  for (const glz_mesh& m : d.meshes) {
    if (m.index_count % 3 != 0) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "mesh index range outside the index buffer";
      return nullptr;
    }
    if (m.material >= d.materials.size()) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "mesh references a missing material";
      return nullptr;
    }
  }
  auto tex_ok = [&](uint32_t id) { return id < d.textures.size(); };
  for (const glz_material& m : d.materials)
    if (!tex_ok(m.diffuse) || !tex_ok(m.roughness) || !tex_ok(m.metalness) || !tex_ok(m.normal) || !tex_ok(m.opacity)) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "material references a missing texture";
      return nullptr;
    }
  if (!s->upload_geometry(err)) return nullptr;
  if (!s->build_materials(err)) return nullptr;
  if (!s->build_lights_and_sky(err)) return nullptr;
  if (!s->build_bvh_as_instance_says(err)) return nullptr;
  if (!hip_ok(hipStreamSynchronize(inst->stream), "scene upload", err)) return nullptr;
  s->info.n_vertices = d.vertices.size();
  s->info.n_triangles = d.indices.size() / 3;
  s->info.n_instances = (uint32_t)s->h_instances.size();
  s->info.n_materials = (uint32_t)d.materials.size();
  s->info.n_lights = s->lights_no;
  s->info.n_rt_lights = (uint32_t)s->h_lights.size();
  s->info.n_textures = (uint32_t)d.textures.size();
  return s.release();
}

bool Scene::upload_geometry(Error& err) {
  hipStream_t st = instance->stream;
  SceneData& d = data;
  static_assert(sizeof(glz_vertex) == 2 * sizeof(float4), "vertex = 2 x float4");
  if (!hip_ok(d_vertices_.upload(reinterpret_cast<const float4*>(d.vertices.data()), d.vertices.size() * 2, st), "upload vertices", err)) return false;
  if (!hip_ok(d_indices_.upload(d.indices.data(), d.indices.size(), st), "upload indices", err)) return false;
  h_instances = rt_instances(d);
  if (!hip_ok(d_instances_.upload(h_instances.data(), h_instances.size(), st), "upload instances", err)) return false;
  inst_base_.assign(h_instances.size(), 0);
  uint64_t total = 0;
  for (size_t i = 0; i < h_instances.size(); ++i) {
    inst_base_[i] = (uint32_t)total;
    total += h_instances[i].index_count / 3;
  }
  if (total >= 0x7FFFFFFFull) {
    err.code = GLZ_E_UNSUPPORTED;
    err.msg = "more than 2^31 world triangles";
    return false;
  }
  info.n_world_triangles = total;
  if (!hip_ok(d_inst_base_.upload(inst_base_.data(), inst_base_.size(), st), "upload instance bases", err)) return false;
  // transforms + inverses (gl_WorldToObjectEXT is supplied by the driver in the reference)
  const std::vector<TransformPair> xf = transform_pairs(d.transforms);
  if (!hip_ok(d_transforms_.upload(xf.data(), xf.size(), st), "upload transforms", err)) return false;
  if (!upload_textures(err)) return false;
  float lut[256];
  for (int i = 0; i < 256; ++i) {   // sRGB EOTF of the R8G8B8A8_SRGB format (scene.rs:1028-1032) [ext]
    const double c = i / 255.0;
    lut[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
  }
  if (!hip_ok(d_srgb_lut_.upload(lut, 256, st), "upload sRGB LUT", err)) return false;
  // calculate_geometric_derivatives (scene.rs:2113-2188)
  uint32_t ntri = 0;
  for (const glz_mesh& m : d.meshes) ntri = std::max<uint32_t>(ntri, (m.index_offset + m.index_count) / 3);
  if (!hip_ok(d_derivatives_.alloc((size_t)ntri * 3), "alloc derivatives", err)) return false;
  if (!hip_ok(launch_derivatives(st, d_vertices_.ptr, d_indices_.ptr, ntri, d_derivatives_.ptr), "derivatives kernel", err)) return false;
  // the host staging vectors above must outlive the async copies
  if (!hip_ok(hipStreamSynchronize(st), "geometry upload", err)) return false;
  dev.vertices = d_vertices_.ptr;
  dev.indices = d_indices_.ptr;
  dev.instances = d_instances_.ptr;
  dev.transforms = d_transforms_.ptr;
  dev.derivatives = d_derivatives_.ptr;
  dev.srgb_lut = d_srgb_lut_.ptr;
  return true;
}

// 128-byte tiles: 8 x 4 RGBA texels or 16 x 8 gray texels (device/shading.h fetch_texel); ragged edges are padded
struct Tiling {
  uint32_t tw, th, bpp, tiles_x, tiles_y;
  Tiling(uint32_t format, uint32_t w, uint32_t h) {
    const bool gray = format == GLZ_TEX_GRAY;
    tw = gray ? 16u : 8u, th = gray ? 8u : 4u, bpp = gray ? 1u : 4u;
    tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
  }
  size_t bytes() const { return (size_t)tiles_x * tiles_y * 128u; }
};
// one image, tiled, appended to `pool` (whose size stays a multiple of 128)
static TexDesc append_tiled(std::vector<uint8_t>& pool, uint32_t format, uint32_t w, uint32_t h, const uint8_t* px) {
  const Tiling t(format, w, h);
  pool.resize((pool.size() + 127) & ~size_t(127));
  const size_t base = pool.size();
  pool.resize(base + t.bytes(), 0);
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      const size_t dst = base + ((size_t)(y / t.th) * t.tiles_x + x / t.tw) * 128u + ((size_t)(y % t.th) * t.tw + x % t.tw) * t.bpp;
      memcpy(&pool[dst], &px[((size_t)y * w + x) * t.bpp], t.bpp);
    }
  return TexDesc{(uint32_t)base, w, h, format | (t.tiles_x << 8)};
}

// Level 0 of every texture in one byte pool (16-byte aligned starts) + a descriptor per texture; what the reference
// keeps as one VkImage per texture behind a descriptor array (scene.rs:1264-1350).
bool Scene::upload_textures(Error& err) {
  hipStream_t st = instance->stream;
  SceneData& d = data;
  std::vector<TexDesc> desc(d.textures.size());
  std::vector<uint8_t> pool;
  for (size_t i = 0; i < d.textures.size(); ++i) {
    const TextureData& t = d.textures[i];
    const size_t bytes = (size_t)t.info.width * t.info.height * (t.info.format == GLZ_TEX_GRAY ? 1 : 4);
    if (t.level0.size() < bytes || t.info.width == 0 || t.info.height == 0 || t.info.format < 1 || t.info.format > 3) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "texture has inconsistent dimensions";
      return false;
    }
    const Tiling tiling(t.info.format, t.info.width, t.info.height);
    if (pool.size() + tiling.bytes() > 0xFFFFFFFFull || tiling.tiles_x >= (1u << 24)) {
      err.code = GLZ_E_UNSUPPORTED;
      err.msg = "texture pool larger than 4 GiB";
      return false;
    }
    if (t.info.width == 1 && t.info.height == 1) {
      // the texel travels in the descriptor (device/shading.h kTexInline): materials' default maps cost no texel load
      uint32_t bits = 0;
      memcpy(&bits, t.level0.data(), tiling.bpp);
      desc[i] = TexDesc{bits, 1u, 1u, t.info.format | 0x80u | (1u << 8)};
      continue;
    }
    desc[i] = append_tiled(pool, t.info.format, t.info.width, t.info.height, t.level0.data());
  }
  if (!hip_ok(d_tex_desc_.upload(desc.data(), desc.size(), st), "upload texture descriptors", err)) return false;
  if (!hip_ok(d_tex_pool_.upload(pool.data(), pool.size(), st), "upload texture pool", err)) return false;
  if (!hip_ok(hipStreamSynchronize(st), "texture upload", err)) return false;   // the staging vectors above must outlive the copies
  dev.tex_desc = d_tex_desc_.ptr;
  dev.tex_pool = d_tex_pool_.ptr;
  dev.n_textures = (uint32_t)d.textures.size();
  // the texels changed: whatever mip levels were built belong to the old ones
  mips_ready_ = false;
  dev.tex_mip_desc = nullptr;
  dev.tex_mip_base = nullptr;
  dev.tex_mip_pool = nullptr;
  h_mips_.clear();
  return true;
}

bool Scene::ensure_mips(Error& err) {
  if (mips_ready_) return true;
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  const size_t nt = data.textures.size();
  h_mips_.assign(nt, {});
  std::vector<std::vector<host::MipLevel>> chains(nt);
  std::vector<std::string> decode_errs(nt);
  auto build_one = [&](size_t i) {
    TextureData& t = data.textures[i];
    if (!t.decode_more_levels(decode_errs[i])) return;   // the file's own levels 1.., still PNG-encoded since parse
    std::vector<host::MipLevel> given(1);
    given[0].width = t.info.width;
    given[0].height = t.info.height;
    given[0].pixels = t.level0;
    for (size_t l = 0; l < t.more_levels.size(); ++l) {
      host::MipLevel m;
      m.width = t.more_dims[2 * l];
      m.height = t.more_dims[2 * l + 1];
      m.pixels = t.more_levels[l];
      given.push_back(std::move(m));
    }
    chains[i] = host::build_mip_chain(t.info.format, std::move(given));
  };
  const unsigned workers = (unsigned)std::min<size_t>(nt, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (workers <= 1) {
    for (size_t i = 0; i < nt; ++i) build_one(i);
  } else {
    std::vector<std::thread> pool;
    std::vector<std::string> failed(workers);
    for (unsigned w = 0; w < workers; ++w)
      pool.emplace_back([&, w] {
        try {
          for (size_t i = w; i < nt; i += workers) build_one(i);
        } catch (const std::exception& ex) {
          failed[w] = ex.what();
        }
      });
    for (auto& th : pool) th.join();
    for (auto& f : failed)
      if (!f.empty()) {
        err.code = GLZ_E_IO;
        err.msg = "mip chain: " + f;
        return false;
      }
  }
  for (size_t i = 0; i < nt; ++i)
    if (!decode_errs[i].empty()) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "Corrupted image: " + decode_errs[i];
      return false;
    }
  std::vector<uint8_t> pool;
  std::vector<TexDesc> desc;
  std::vector<uint32_t> base(nt, 0);
  for (size_t i = 0; i < nt; ++i) {
    const uint32_t levels = (uint32_t)chains[i].size();
    base[i] = (uint32_t)desc.size() | (levels << 24);
    for (uint32_t l = 1; l < levels; ++l) {
      const host::MipLevel& m = chains[i][l];
      desc.push_back(append_tiled(pool, data.textures[i].info.format, m.width, m.height, m.pixels.data()));
      h_mips_[i].push_back(m.pixels);
    }
    if (pool.size() > 0xFFFFFFF0ull || desc.size() >= (1u << 24)) {
      err.code = GLZ_E_UNSUPPORTED;
      err.msg = "mip pool larger than 4 GiB";
      return false;
    }
  }
  hipStream_t st = instance->stream;
  if (!hip_ok(d_tex_mip_desc_.upload(desc.data(), desc.size(), st), "upload mip descriptors", err)) return false;
  if (!hip_ok(d_tex_mip_pool_.upload(pool.data(), pool.size(), st), "upload mip pool", err)) return false;
  if (!hip_ok(d_tex_mip_base_.upload(base.data(), base.size(), st), "upload mip table", err)) return false;
  if (!hip_ok(hipStreamSynchronize(st), "mip upload", err)) return false;
  dev.tex_mip_desc = d_tex_mip_desc_.ptr;
  dev.tex_mip_pool = d_tex_mip_pool_.ptr;
  dev.tex_mip_base = d_tex_mip_base_.ptr;
  mips_ready_ = true;
  return true;
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
  if (level - 1 >= h_mips_[texture].size()) return true;
  pixels = h_mips_[texture][level - 1];
  w = host::mip_dim(t.info.width, level);
  h = host::mip_dim(t.info.height, level);
  return true;
}

// load_raytrace_materials_to_gpu (scene.rs:1821-1860)
bool Scene::build_materials(Error& err) {
  h_materials.clear();
  for (const glz_material& m : data.materials) {
    RTMaterial r{};
    for (int i = 0; i < 3; ++i) {
      r.diffuse_mul[i] = (float)m.diffuse_mul[i] / 255.0f;   // col_int_to_f32, scene.rs:1930-1937
      r.emissive_col[i] = m.has_emissive ? (float)m.emissive_col[i] / 255.0f : 0.0f;
    }
    r.diffuse_mul[3] = r.emissive_col[3] = 1.0f;
    const unsigned metal = m.metal < GLZ_METAL_COUNT ? m.metal : 0;
    for (int i = 0; i < 16; ++i) {
      const float n = GLZ_METAL_N[metal][i], k = GLZ_METAL_K[metal][i];
      r.metal_ior.w[i] = n;
      r.metal_fresnel.w[i] = (n * n) + (k * k);
    }
    r.diffuse = m.diffuse;
    r.roughness = m.roughness;
    r.metalness = m.metalness;
    r.opacity = m.opacity;
    r.normal = m.normal;
    r.bsdf_index = sbt_callable_index(m.mtype);
    r.roughness_mul = m.roughness_mul;
    r.metalness_mul = m.metalness_mul;
    r.anisotropy = m.anisotropy;
    r.ior_dielectric = m.ior;
    r.is_specular = (m.mtype == GLZ_MAT_MIRROR || m.mtype == GLZ_MAT_GLASS) ? 1u : 0u;   // material.rs:103-114
    r.is_emissive = m.has_emissive ? 1u : 0u;
    h_materials.push_back(r);
  }
  if (!hip_ok(d_materials_.upload(h_materials.data(), h_materials.size(), instance->stream), "upload materials", err)) return false;
  if (!hip_ok(hipStreamSynchronize(instance->stream), "materials upload", err)) return false;
  dev.materials = d_materials_.ptr;
  dev.n_materials = (uint32_t)h_materials.size();
  dev.has_non_opaque = 0u;   // which k_trace runs (launch_trace): the one without alpha code, or the one with the alpha phase
  for (const RTMaterial& m : h_materials) dev.has_non_opaque |= m.opacity != 0u ? 1u : 0u;
  return true;
}

// reorder_lights (scene.rs:628-635), load_raytrace_lights_to_gpu (:1863-1927),
// calculate_skymap_distributions + build_sky_raytrace_buffers (:2191-2313)
bool Scene::build_lights_and_sky(Error& err) {
  hipStream_t st = instance->stream;
  std::vector<glz_light> ordered;
  const glz_light* sky = nullptr;
  for (const glz_light& l : data.lights) {
    if (l.ltype > GLZ_LIGHT_SKY) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "Invalid enum value for LightType";
      return false;
    }
    if (l.ltype == GLZ_LIGHT_SKY) { if (!sky) sky = &l; }
    else ordered.push_back(l);
  }
  const bool has_sky = sky != nullptr;
  if (sky) ordered.push_back(*sky);
  lights_no = (uint32_t)ordered.size();   // scene.rs:1549 -- NOT the number of expanded RTLights
  h_lights.clear();
  for (const glz_light& l : ordered) {
    RTLight r{};
    memcpy(r.color.w, l.color, 64);
    float dx = l.direction[0], dy = l.direction[1], dz = l.direction[2];
    if (dx == 0.0f && dy == 0.0f && dz == 0.0f) dy = -1.0f;
    // the reference calls `dir.normalize()` and drops the result: directions stay un-normalised (Q14)
    r.pos[0] = l.position[0]; r.pos[1] = l.position[1]; r.pos[2] = l.position[2];
    r.dir[0] = dx; r.dir[1] = dy; r.dir[2] = dz;
    r.shader = l.ltype;   // sbt_callable_index, light.rs:111-119
    r.instance_id = 0xFFFFFFFFu;
    r.intensity = l.intensity;
    r.delta = (l.ltype == GLZ_LIGHT_OMNI || l.ltype == GLZ_LIGHT_SUN) ? 1u : 0u;
    if (l.ltype == GLZ_LIGHT_AREA) {
      // one RTLight per instance whose mesh uses the emitting material (map_materials_to_instances, :1764-1781)
      const uint16_t material_id = (uint16_t)l.resource_id;
      std::vector<uint32_t> ids;
      for (size_t i = 0; i < data.instances.size(); ++i) {
        const glz_mesh* found = mesh_by_id(data, data.instances[i].mesh_id);
        if (found && found->material == material_id) ids.push_back((uint32_t)(uint16_t)i);
      }
      if (ids.empty()) ids.push_back(0);
      for (uint32_t id : ids) {
        if (id >= h_instances.size()) {
          err.code = GLZ_E_INVALID_DATA;
          err.msg = "area light refers to a missing instance";
          return false;
        }
        r.instance_id = id;
        h_lights.push_back(r);
      }
    } else {
      h_lights.push_back(r);
    }
  }
  if (h_lights.empty()) {   // dummy light so the buffer is never empty (:1906-1918)
    RTLight r{};
    r.instance_id = 0xFFFFFFFFu;
    r.intensity = 1.0f;
    r.delta = 1u;
    h_lights.push_back(r);
  }
  if (!hip_ok(d_lights_.upload(h_lights.data(), h_lights.size(), st), "upload lights", err)) return false;
  dev.lights = d_lights_.ptr;
  dev.n_rt_lights = (uint32_t)h_lights.size();

  // sky: Light::default() when the scene has none (scene.rs:2249)
  glz_light dflt{};
  dflt.intensity = 1.0f;
  const glz_light& sl = has_sky ? ordered.back() : dflt;
  if (sl.resource_id >= data.textures.size()) {
    err.code = GLZ_E_INVALID_DATA;
    err.msg = "sky light references a missing texture";
    return false;
  }
  float rot32[16];
  host::sky_rotation(sl.yaw_deg, sl.pitch_deg, sl.roll_deg).to_f32(rot32);   // Matrix4<f32> in the reference
  host::Mat4d inv;
  if (!host::invert(host::Mat4d::from_f32(rot32), inv)) inv = host::Mat4d::identity();
  memcpy(h_sky.obj2world, rot32, 64);
  inv.to_f32(h_sky.world2obj);
  h_sky.tex_id = sl.resource_id;
  h_sky.intensity = sl.intensity;
  if (sky_distribution_tex_ != h_sky.tex_id) {
    // recalculated only when the sky texture changes (scene.rs:2256-2260)
    const TextureData& map = data.textures[h_sky.tex_id];
    const uint32_t W = map.info.width, H = map.info.height;
    const size_t bpp = map.info.format == GLZ_TEX_GRAY ? 1 : 4;
    std::vector<float> values((size_t)W * H);
    const float pi = 3.14159265358979323846f;
    for (uint32_t y = 0; y < H; ++y) {
      const float sint = sinf(pi * ((float)y + 0.5f) / (float)H);
      const uint8_t* row = map.level0.data() + (size_t)y * W * bpp;
      for (uint32_t x = 0; x < W; ++x) {
        const uint8_t* p = row + x * bpp;
        const float r = (float)p[0] / 255.0f, g = (float)p[bpp > 1 ? 1 : 0] / 255.0f, b = (float)p[bpp > 1 ? 2 : 0] / 255.0f;
        values[(size_t)y * W + x] = host::illuminant_luminance(r, g, b) * sint;
      }
    }
    std::vector<float> cond_cdf, integrals(H), marginal_cdf;
    cond_cdf.reserve((size_t)(W + 1) * H);
    for (uint32_t y = 0; y < H; ++y) integrals[y] = host::distribution1d(values.data() + (size_t)y * W, W, cond_cdf);
    h_sky_header.marginal_integral = host::distribution1d(integrals.data(), H, marginal_cdf);
    h_sky_header.marginal_cdf_count = H + 1;
    h_sky_header.conditional_integral_offset = H + (H + 1);
    h_sky_header.conditional_cdf_count = W + 1;
    h_sky_marginal = marginal_cdf;
    h_sky_marginal.insert(h_sky_marginal.end(), integrals.begin(), integrals.end());   // marginal values
    h_sky_marginal.insert(h_sky_marginal.end(), integrals.begin(), integrals.end());   // conditional integrals
    if (!hip_ok(d_sky_marginal_.upload(h_sky_marginal.data(), h_sky_marginal.size(), st), "upload sky marginal", err)) return false;
    if (!hip_ok(d_sky_cond_values_.upload(values.data(), values.size(), st), "upload sky values", err)) return false;
    if (!hip_ok(d_sky_cond_cdf_.upload(cond_cdf.data(), cond_cdf.size(), st), "upload sky cdf", err)) return false;
    if (!hip_ok(hipStreamSynchronize(st), "sky upload", err)) return false;
    dev.sky_w = W;
    dev.sky_h = H;
    sky_distribution_tex_ = h_sky.tex_id;
  }
  if (!hip_ok(hipStreamSynchronize(st), "lights upload", err)) return false;
  dev.sky = h_sky;
  dev.sky_header = h_sky_header;
  dev.sky_marginal = d_sky_marginal_.ptr;
  dev.sky_cdf = d_sky_marginal_.ptr;
  dev.sky_cond_values = d_sky_cond_values_.ptr;
  dev.sky_cond_cdf = d_sky_cond_cdf_.ptr;
  return true;
}

// ---- instance boxes of the top level: world AABB of the mesh's VERTICES under the instance's transform, padded.  (The eight corners
// of the mesh's object box, which is what a top level normally takes, give a box up to sqrt(2) too wide per axis for a rotated
// instance -- a quarter more instance entries per ray in the column forest.  The vertices cost instances x vertices; past `budget`
// point transforms the remaining instances fall back to the corners.) ----
std::vector<std::vector<float>> mesh_points(const SceneData& d, const std::vector<std::pair<uint32_t, uint32_t>>& ranges) {
  std::vector<std::vector<float>> out(ranges.size());   // xyz of the vertices a mesh references, once each, in first-use order
  std::vector<uint8_t> seen(d.vertices.size(), 0);
  for (size_t mi = 0; mi < ranges.size(); ++mi) {
    const uint32_t off = ranges[mi].first, count = ranges[mi].second;
    std::vector<float>& pts = out[mi];
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t v = d.indices[off + k];
      if (seen[v]) continue;
      seen[v] = 1;
      pts.insert(pts.end(), d.vertices[v].vv, d.vertices[v].vv + 3);
    }
    for (uint32_t k = 0; k < count; ++k) seen[d.indices[off + k]] = 0;
  }
  return out;
}

std::vector<uint8_t> exact_box_instances(const std::vector<uint32_t>& mesh_of, const std::vector<uint64_t>& mesh_point_count, uint64_t budget) {
  std::vector<uint8_t> exact(mesh_of.size(), 0);
  uint64_t spent = 0;
  for (size_t i = 0; i < mesh_of.size(); ++i) {
    const uint64_t n = mesh_point_count[mesh_of[i]];
    if (n != 0 && spent + n <= budget) {
      spent += n;
      exact[i] = 1;
    }
  }
  return exact;
}

void host_instance_boxes(const std::vector<uint32_t>& mesh_of, const std::vector<uint32_t>& transform_of, const std::vector<InstanceBoxMesh>& meshes,
                         const std::vector<glz_transform>& transforms, uint64_t budget, std::vector<float4>& blo, std::vector<float4>& bhi) {
  const size_t ni = mesh_of.size();
  blo.assign(ni, float4{});
  bhi.assign(ni, float4{});
  std::vector<uint64_t> counts(meshes.size());
  for (size_t m = 0; m < meshes.size(); ++m) counts[m] = meshes[m].points.size() / 3;
  const std::vector<uint8_t> exact = exact_box_instances(mesh_of, counts, budget);
  for (size_t i = 0; i < ni; ++i) {
    const InstanceBoxMesh& m = meshes[mesh_of[i]];
    const float* M = transforms[transform_of[i]].m;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto take = [&](double x, double y, double z) {
      for (int k = 0; k < 3; ++k) {
        const double w = (double)M[k] * x + (double)M[4 + k] * y + (double)M[8 + k] * z + (double)M[12 + k];
        lo[k] = std::min(lo[k], w);
        hi[k] = std::max(hi[k], w);
      }
    };
    const std::vector<float>& pts = m.points;
    if (exact[i]) {
      for (size_t k = 0; k + 2 < pts.size(); k += 3) take(pts[k], pts[k + 1], pts[k + 2]);
    } else {
      for (int c = 0; c < 8; ++c) take((c & 1) ? m.hi[0] : m.lo[0], (c & 2) ? m.hi[1] : m.lo[1], (c & 4) ? m.hi[2] : m.lo[2]);
    }
    float l[3], h[3];
    for (int k = 0; k < 3; ++k) {
      if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0;   // a mesh without triangles / non-finite transform: a point nobody hits
      // the tracer's world vertices are single-precision sums of four terms: four roundings of the largest one can get
      const double mag = std::fabs((double)M[k]) * std::max(std::fabs((double)m.lo[0]), std::fabs((double)m.hi[0])) +
                         std::fabs((double)M[4 + k]) * std::max(std::fabs((double)m.lo[1]), std::fabs((double)m.hi[1])) +
                         std::fabs((double)M[8 + k]) * std::max(std::fabs((double)m.lo[2]), std::fabs((double)m.hi[2])) + std::fabs((double)M[12 + k]);
      const double pad = 1e-5 * std::max({std::fabs(lo[k]), std::fabs(hi[k]), 1e-3}) + 1e-6 * (hi[k] - lo[k]) + (std::isfinite(mag) ? 4.8e-7 * mag : 0.0);
      l[k] = std::nextafterf((float)(lo[k] - pad), -INFINITY);
      h[k] = std::nextafterf((float)(hi[k] + pad), INFINITY);
    }
    blo[i] = make_float4(l[0], l[1], l[2], 0.0f);
    bhi[i] = make_float4(h[0], h[1], h[2], 0.0f);
  }
}

// how far from the origin the instances reach: the diagonal of their boxes' union plus its largest coordinate (TlasInstance::slack)
double instance_reach(const std::vector<float4>& blo, const std::vector<float4>& bhi) {
  double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
  for (size_t i = 0; i < blo.size(); ++i) {
    const float l[3] = {blo[i].x, blo[i].y, blo[i].z}, h[3] = {bhi[i].x, bhi[i].y, bhi[i].z};
    for (int k = 0; k < 3; ++k) {
      wlo[k] = std::min(wlo[k], (double)l[k]);
      whi[k] = std::max(whi[k], (double)h[k]);
    }
  }
  return std::sqrt((whi[0] - wlo[0]) * (whi[0] - wlo[0]) + (whi[1] - wlo[1]) * (whi[1] - wlo[1]) + (whi[2] - wlo[2]) * (whi[2] - wlo[2])) +
         std::max({std::fabs(wlo[0]), std::fabs(wlo[1]), std::fabs(wlo[2]), std::fabs(whi[0]), std::fabs(whi[1]), std::fabs(whi[2])});
}

// Two-level structure (types.h TlasInstance; acceleration.rs:319-345: a BLAS per mesh, a TLAS over the instances).  The meshes'
// hierarchies are built by the ordinary builder over ONE pseudo-instance with the identity transform (object space = its "world"),
// the top level by the same builder over the instances' world boxes (HierarchyInputs::given_lo).  Memory is O(meshes + instances).
bool Scene::build_two_level(Error& err) {
  hipStream_t st = instance->stream;
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  h_mesh_ranges.clear();
  // ---- unique meshes (index ranges) ----
  std::vector<uint32_t> mesh_of;
  std::vector<MeshBuild> meshes;
  uint64_t total_tris = 0;
  for (const std::pair<uint32_t, uint32_t>& range : unique_meshes(h_instances, mesh_of)) {
    meshes.emplace_back();
    meshes.back().mesh.index_offset = range.first;
    meshes.back().mesh.index_count = range.second;
    meshes.back().range.tri_base = (uint32_t)total_tris;
    total_tris += range.second / 3u;
  }
  if (total_tris >= 0x3FFFFFFFull) {
    err.code = GLZ_E_UNSUPPORTED;
    err.msg = "more than 2^30 mesh triangles";
    return false;
  }
  const uint32_t nt = (uint32_t)total_tris;
  d_nodes_.release();
  if (!hip_ok(d_tris_.alloc((size_t)nt + 1), "alloc BVH triangles", err)) return false;
  if (!hip_ok(hipMemsetAsync(d_tris_.ptr + nt, 0, sizeof(BvhTri), st), "clear BVH triangle padding", err)) return false;
  if (!hip_ok(d_shade_tris_.alloc((size_t)nt * 8), "alloc shading records", err)) return false;
  // helpers of the per-mesh builds: an identity transform, an opaque material (the opacity flag is per instance here)
  DeviceBuffer<TransformPair> d_ident;
  DeviceBuffer<RTMaterial> d_opaque;
  DeviceBuffer<RTInstance> d_pseudo;
  DeviceBuffer<uint32_t> d_zero, d_one;
  {
    TransformPair ident{};
    for (int k = 0; k < 4; ++k) ident.o2w[5 * k] = ident.w2o[5 * k] = 1.0f;
    RTMaterial opaque{};
    const uint32_t zero = 0u, one = 1u;
    if (!hip_ok(d_ident.upload(&ident, 1, st), "upload", err) || !hip_ok(d_opaque.upload(&opaque, 1, st), "upload", err) ||
        !hip_ok(d_zero.upload(&zero, 1, st), "upload", err) || !hip_ok(d_one.upload(&one, 1, st), "upload", err) || !hip_ok(d_pseudo.alloc(1), "alloc", err))
      return false;
    if (!hip_ok(hipStreamSynchronize(st), "upload", err)) return false;
  }
  tl_mesh_depth_ = 0;
  for (MeshBuild& m : meshes) {
    const uint32_t n = m.mesh.index_count / 3u;
    if (n == 0) continue;
    const RTInstance pseudo{m.mesh.index_offset, m.mesh.index_count, 0u, 0u};
    if (!hip_ok(hipMemcpyAsync(d_pseudo.ptr, &pseudo, sizeof(pseudo), hipMemcpyHostToDevice, st), "upload", err) || !hip_ok(hipStreamSynchronize(st), "upload", err))
      return false;
    HierarchyInputs in{d_vertices_.ptr, d_indices_.ptr, d_pseudo.ptr, d_zero.ptr, 1u, d_ident.ptr, d_opaque.ptr, n, build_opts_.builder, build_opts_.pair_area_ratio};
    in.emit_quads = true;   // 64-byte leaf records (object space here), leaf links ~leaf number relative to the mesh
    HierarchyOutputs out{};
    DeviceBuffer<BvhTri> tris;
    if (!hip_ok(tris.alloc((size_t)n + 1), "alloc mesh triangles", err)) return false;
    out.tris = tris.ptr;
    if (!hip_ok(build_hierarchy(st, in, out), "mesh hierarchy", err)) return false;
    m.nodes = std::move(out.nodes);
    m.quads = std::move(out.quads);   // the mesh's leaf records (object space)
    m.mesh.grid = out.grid;
    for (int k = 0; k < 3; ++k) { m.mesh.lo[k] = out.bounds_lo[k]; m.mesh.hi[k] = out.bounds_hi[k]; }
    tl_mesh_depth_ = std::max(tl_mesh_depth_, out.depth);
    // the mesh's triangles and per-object-triangle shading records go to their place in the concatenated arrays
    if (!hip_ok(hipMemcpyAsync(d_tris_.ptr + m.range.tri_base, tris.ptr, sizeof(BvhTri) * n, hipMemcpyDeviceToDevice, st), "copy mesh triangles", err) ||
        !hip_ok(launch_shade_records(st, n, tris.ptr, d_pseudo.ptr, d_indices_.ptr, d_vertices_.ptr, d_derivatives_.ptr, d_one.ptr,
                                     d_shade_tris_.ptr + 8 * (size_t)m.range.tri_base), "k_shade_records", err) ||
        !hip_ok(hipStreamSynchronize(st), "mesh hierarchy", err))
      return false;
  }
  // ---- where each mesh's nodes and leaf records go: one array each (TlasInstance::node_base / quad_base); the nodes follow a top
  // level that does not exist yet ----
  uint32_t total_leaves = 0;
  tl_top_nodes_ = 0;
  uint32_t at = 0;
  for (MeshBuild& m : meshes) {
    m.range.node_base = at;
    m.range.n_nodes = (uint32_t)m.nodes.count;
    m.range.quad_base = total_leaves;
    at += m.range.n_nodes ? m.range.n_nodes : 1u;   // a mesh without triangles gets one node without children: entering it finds nothing
    total_leaves += (uint32_t)m.quads.count;
  }
  d_quads_.release();
  if (!hip_ok(d_quads_.alloc((size_t)total_leaves + 1), "alloc leaf records", err) ||
      !hip_ok(hipMemsetAsync(d_quads_.ptr + total_leaves, 0, sizeof(BvhQuad), st), "clear leaf record padding", err))
    return false;
  for (const MeshBuild& m : meshes)
    if (m.quads.count && !hip_ok(hipMemcpyAsync(d_quads_.ptr + m.range.quad_base, m.quads.ptr, sizeof(BvhQuad) * m.quads.count, hipMemcpyDeviceToDevice, st), "copy leaf records", err))
      return false;
  // ---- what the top level needs of each mesh, kept for update_transforms ----
  tl_meshes_.clear();
  for (const MeshBuild& m : meshes) {
    tl_meshes_.push_back(m.mesh);
    h_mesh_ranges.push_back(m.range);
  }
  tl_mesh_of_ = mesh_of;
  tl_points_ready_ = false;
  // ---- instance boxes (host_instance_boxes), then the top level over them ----
  const size_t ni = h_instances.size();
  std::vector<float4> blo, bhi;
  host_instance_boxes(tl_mesh_of_, instance_transforms(), box_meshes(), data.transforms, kExactBoxBudget, blo, bhi);
  DeviceBuffer<float4> d_blo, d_bhi;
  if (!hip_ok(d_blo.upload(blo.data(), ni, st), "upload instance boxes", err) || !hip_ok(d_bhi.upload(bhi.data(), ni, st), "upload instance boxes", err) ||
      !hip_ok(hipStreamSynchronize(st), "upload instance boxes", err))
    return false;
  return assemble_top_level(d_blo.ptr, d_bhi.ptr, blo, bhi, &meshes, timer, err);
}

// Everything from "the instance boxes are on the device" onwards, for a new scene and for moved instances alike: the hierarchy over
// the boxes, its nodes in front of the meshes' nodes in one array, the instance records in its leaf order, the top table, info.
// h_lo / h_hi: host copies of the boxes; empty = read back here.  built: the meshes' nodes as a build has just left them (their
// place in the array: h_mesh_ranges, behind tl_top_nodes_ = 0 top nodes), or null = they sit in d_nodes_ behind the old top level.
// timer: started by the caller, where info.build_ms is to begin.
bool Scene::assemble_top_level(const float4* d_lo, const float4* d_hi, std::vector<float4>& h_lo, std::vector<float4>& h_hi, const std::vector<MeshBuild>* built,
                               StreamTimer& timer, Error& err) {
  hipStream_t st = instance->stream;
  const size_t ni = h_instances.size();
  DeviceBuffer<BvhTri> top_tris;
  HierarchyOutputs top{};
  if (!hip_ok(top_tris.alloc(ni + 1), "alloc", err)) return false;
  {
    HierarchyInputs in{nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr, (uint32_t)ni, build_opts_.builder, 0.0f};
    in.given_lo = d_lo;
    in.given_hi = d_hi;
    top.tris = top_tris.ptr;
    if (!hip_ok(build_hierarchy(st, in, top), "instance hierarchy", err)) return false;
  }
  // ---- one node array: top level first, then the meshes (moved as they are when the top level's size changes) ----
  const MeshRange& last = h_mesh_ranges.back();   // (a two-level scene has a mesh)
  const uint32_t old_top = tl_top_nodes_, new_top = (uint32_t)top.nodes.count;
  const uint32_t mesh_nodes = last.node_base + (last.n_nodes ? last.n_nodes : 1u) - old_top, n_nodes = new_top + mesh_nodes;
  if (n_nodes >= (uint32_t)kBvhTopFlag) {
    err.code = GLZ_E_UNSUPPORTED;
    err.msg = "more than 2^30 BVH nodes";
    return false;
  }
  DeviceBuffer<BvhNode4> fresh;
  const bool in_place = !built && new_top == old_top;
  if (!in_place && !hip_ok(fresh.alloc(n_nodes), "alloc nodes", err)) return false;
  BvhNode4* nodes = in_place ? d_nodes_.ptr : fresh.ptr;
  bool ok = !new_top || hip_ok(hipMemcpyAsync(nodes, top.nodes.ptr, sizeof(BvhNode4) * new_top, hipMemcpyDeviceToDevice, st), "copy nodes", err);
  if (built) {
    static const BvhNode4 childless = childless_node4();   // (static: the copy below is asynchronous)
    for (const MeshBuild& m : *built) {
      BvhNode4* to = nodes + new_top + m.range.node_base;
      if (ok && m.nodes.count) ok = hip_ok(hipMemcpyAsync(to, m.nodes.ptr, sizeof(BvhNode4) * m.nodes.count, hipMemcpyDeviceToDevice, st), "copy nodes", err);
      if (ok && !m.nodes.count) ok = hip_ok(hipMemcpyAsync(to, &childless, sizeof(BvhNode4), hipMemcpyHostToDevice, st), "copy nodes", err);
    }
  } else if (!in_place && ok) {
    ok = hip_ok(hipMemcpyAsync(nodes + new_top, d_nodes_.ptr + old_top, sizeof(BvhNode4) * mesh_nodes, hipMemcpyDeviceToDevice, st), "move mesh nodes", err);
  }
  // instance records in the top level's leaf order
  std::vector<BvhTri> order(ni);
  if (ok) ok = hip_ok(hipMemcpyAsync(order.data(), top_tris.ptr, sizeof(BvhTri) * ni, hipMemcpyDeviceToHost, st), "read instance order", err);
  if (h_lo.empty()) {
    h_lo.resize(ni);
    h_hi.resize(ni);
    if (ok) ok = hip_ok(hipMemcpyAsync(h_lo.data(), d_lo, sizeof(float4) * ni, hipMemcpyDeviceToHost, st), "read instance boxes", err);
    if (ok) ok = hip_ok(hipMemcpyAsync(h_hi.data(), d_hi, sizeof(float4) * ni, hipMemcpyDeviceToHost, st), "read instance boxes", err);
  }
  if (!hip_ok(hipStreamSynchronize(st), "top level", err) || !ok) return false;
  if (!in_place) {
    d_nodes_ = std::move(fresh);
    for (MeshRange& r : h_mesh_ranges) r.node_base = r.node_base - old_top + new_top;
  }
  tl_top_nodes_ = new_top;
  if (!write_top_records(order, instance_reach(h_lo, h_hi), err)) return false;
  if (!d_top_.ptr && !hip_ok(d_top_.alloc(kBvhTopNodes), "alloc BVH top table", err)) return false;
  if (!hip_ok(launch_top_table(st, d_nodes_.ptr, new_top, d_top_.ptr), "k_top_table", err)) return false;   // unused by the two-level tracer, kept valid
  timer.stop(st);
  if (!hip_ok(hipStreamSynchronize(st), "top level", err)) return false;
  finish_two_level(top, timer.ms());
  return true;
}

// The TlasInstance records in the top level's leaf order (`order`: the top level's leaves, world_id = instance), and the transform
// flags.  `reach`: instance_reach of the instance boxes the top level was built over.
bool Scene::write_top_records(const std::vector<BvhTri>& order, double reach, Error& err) {
  hipStream_t st = instance->stream;
  const size_t ni = h_instances.size();
  std::vector<TlasInstance> recs(ni);
  const std::vector<TransformPair> xf = transform_pairs(data.transforms);
  for (size_t s = 0; s < ni; ++s) {
    const uint32_t i = order[s].world_id;   // the box this leaf was built from
    const RTInstance& in = h_instances[i];
    const TlMesh& m = tl_meshes_[tl_mesh_of_[i]];
    const MeshRange& mr = h_mesh_ranges[tl_mesh_of_[i]];
    const TransformPair& T = xf[in.transform_id];
    TlasInstance r{};
    for (int row = 0; row < 3; ++row)
      for (int col = 0; col < 4; ++col) r.w2o[4 * row + col] = T.w2o[4 * col + row];   // rows of the column-major inverse
    memcpy(r.o2w, T.o2w, 64);
    r.grid = m.grid;
    // slack of the object-space box tests: rounding of the transformed ray (relative to where in the world it can be) and of
    // the triangle's world position, taken back to object units; generous (x 32)
    double wnorm = 0.0, tr = 0.0, objmax = 0.0;
    for (int row = 0; row < 3; ++row) {
      wnorm = std::max(wnorm, std::fabs((double)r.w2o[4 * row]) + std::fabs((double)r.w2o[4 * row + 1]) + std::fabs((double)r.w2o[4 * row + 2]));
      tr = std::max(tr, std::fabs((double)r.w2o[4 * row + 3]));
      objmax = std::max({objmax, std::fabs((double)m.lo[row]), std::fabs((double)m.hi[row])});
    }
    const double eps = 1.1920929e-7;
    // (in object units: the tracer turns it into cells of each axis -- a thin mesh has tiny cells across its thin side, and the pad
    // that side needs, taken for all three, would make every box of the mesh as wide as the mesh)
    r.slack = (float)(32.0 * eps * (wnorm * reach + tr + objmax));
    r.w2o_norm = (float)wnorm;   // the tracer adds 32 eps wnorm |o|_1 per ray: origins far outside the scene's bounds
    r.node_base = mr.node_base;
    r.tri_base = mr.tri_base;
    r.quad_base = mr.quad_base;
    r.world_base = inst_base_[i];
    r.instance = i;
    r.non_opaque = h_materials[in.material_id].opacity != 0 ? 1u : 0u;
    recs[s] = r;
  }
  if (!hip_ok(d_tlas_instances_.upload(recs.data(), ni, st), "upload instance records", err)) return false;
  const std::vector<uint32_t> ident = identity_flags(data.transforms);
  if (!hip_ok(d_xf_identity_.upload(ident.data(), ident.size(), st), "upload transform flags", err)) return false;
  return hip_ok(hipStreamSynchronize(st), "upload instance records", err);   // the staging vectors above must outlive the copies
}

// info, stack bound and DeviceScene of a two-level scene whose node array (top level first) and records are in place
void Scene::finish_two_level(const HierarchyOutputs& top, float build_ms) {
  const uint32_t n_nodes = (uint32_t)d_nodes_.count, nt = (uint32_t)(d_tris_.count - 1), ni = (uint32_t)h_instances.size();
  info.bvh_nodes = n_nodes;
  info.bvh_depth = top.depth + tl_mesh_depth_;
  info.bvh_sah_cost = top.sah;
  info.build_ms = build_ms;
  for (int k = 0; k < 3; ++k) {
    info.bounds_min[k] = top.bounds_lo[k];
    info.bounds_max[k] = top.bounds_hi[k];
    info.bvh_grid_lo[k] = top.grid.lo[k];
    info.bvh_grid_cell[k] = top.grid.cell[k];
  }
  // both levels' entries and one exit marker share the stack
  const uint32_t stack_bound = 3u * (top.depth + tl_mesh_depth_) + 2u;
  stack_overflow_depth = stack_bound > (uint32_t)kTraversalLdsStack ? stack_bound - kTraversalLdsStack + 1 : 1;
  dev.transforms = d_transforms_.ptr;
  dev.bvh_nodes = d_nodes_.ptr;
  dev.bvh_top = d_top_.ptr;
  dev.bvh_grid = top.grid;
  dev.bvh_tris = d_tris_.ptr;
  dev.bvh_quads = d_quads_.ptr;   // the meshes' leaf records, concatenated
  dev.shade_tris = d_shade_tris_.ptr;
  dev.tlas_nodes = d_nodes_.ptr;
  dev.tlas_instances = d_tlas_instances_.ptr;
  dev.xf_identity = d_xf_identity_.ptr;
  dev.two_level = 1u;
  d_nodes8_.release();   // (the two-level tracer walks 4-wide nodes only)
  dev.bvh_nodes8 = nullptr;
  info.bvh_nodes8 = 0;
  dev.n_world_tris = (uint32_t)info.n_world_triangles;
  info.as_levels = 2;
  info.n_as_triangles = nt;
  info.as_bytes = (uint64_t)n_nodes * sizeof(BvhNode4) + (uint64_t)(nt + 1) * sizeof(BvhTri) + (uint64_t)nt * 128u + (uint64_t)ni * sizeof(TlasInstance) +
                  (uint64_t)d_quads_.count * sizeof(BvhQuad);
}

// The structure with the instance's current options; from then on they are the scene's own (update_transforms keeps them)
bool Scene::build_bvh_as_instance_says(Error& err) {
  build_opts_ = BuildOptions{instance->bvh_builder, instance->bvh_pair_area_ratio, instance->as_levels};
  if (!build_bvh(err)) return false;
  build_opts_.as_levels = (int)info.as_levels;   // the shape built
  return true;
}

bool Scene::build_bvh(Error& err) {
  // instanced scenes keep one hierarchy per mesh (acceleration.rs:319-345) instead of one over every instanced triangle
  {
    uint64_t unique = 0;
    std::vector<uint32_t> mesh_of;
    for (const std::pair<uint32_t, uint32_t>& range : unique_meshes(h_instances, mesh_of)) unique += range.second / 3u;
    const bool wanted = build_opts_.as_levels == 2 || (build_opts_.as_levels == 0 && unique > 0 && info.n_world_triangles > 4 * unique);
    dev.two_level = 0u;
    dev.tlas_nodes = nullptr;
    dev.tlas_instances = nullptr;
    if (wanted && info.n_world_triangles > 0) return build_two_level(err);
  }
  hipStream_t st = instance->stream;
  const uint32_t n = (uint32_t)info.n_world_triangles;
  d_nodes_.release();
  if (!hip_ok(d_tris_.alloc((size_t)n + 1), "alloc BVH triangles", err)) return false;   // + 1: the tracer loads a leaf's partner slot unconditionally
  if (!hip_ok(hipMemsetAsync(d_tris_.ptr + n, 0, sizeof(BvhTri), st), "clear BVH triangle padding", err)) return false;
  HierarchyInputs in{d_vertices_.ptr, d_indices_.ptr, d_instances_.ptr, d_inst_base_.ptr, (uint32_t)h_instances.size(), d_transforms_.ptr,
                d_materials_.ptr, n, build_opts_.builder, build_opts_.pair_area_ratio};
  in.emit_quads = true;   // the flattened tracer reads one 64-byte record per leaf (types.h BvhQuad); leaf links are ~leaf number
  in.emit_wide8 = true;   // ... and a small tile share the same hierarchy eight wide (types.h BvhNode8, k_trace8)
  HierarchyOutputs out{};
  out.tris = d_tris_.ptr;
  d_quads_.release();
  d_nodes8_.release();
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  const hipError_t be = build_hierarchy(st, in, out);
  timer.stop(st);
  const float ms = timer.ms();
  if (!hip_ok(be, "hierarchy build", err)) return false;
  d_quads_ = std::move(out.quads);
  d_nodes8_ = std::move(out.nodes8);
  d_nodes_ = std::move(out.nodes);   // allocated by the build once the number of 4-wide nodes is known
  const uint32_t n_nodes = (uint32_t)d_nodes_.count;
  info.bvh_nodes = n_nodes;
  info.bvh_depth = out.depth;
  info.bvh_sah_cost = out.sah;
  info.build_ms = ms;
  for (int k = 0; k < 3; ++k) {
    info.bounds_min[k] = out.bounds_lo[k];
    info.bounds_max[k] = out.bounds_hi[k];
  }
  // traversal stack: kTraversalLdsStack levels live in LDS, the rest spills to a per-lane HBM area
  // (a 4-wide visit pushes up to three siblings, so the bound is 3 entries per level)
  const uint32_t stack_bound = std::max(3u * out.depth, 7u * out.depth8) + 1u;   // (an 8-wide visit pushes up to seven)
  stack_overflow_depth = stack_bound > (uint32_t)kTraversalLdsStack ? stack_bound - kTraversalLdsStack + 1 : 1;
  dev.bvh_nodes = d_nodes_.ptr;
  if (n_nodes >= (uint32_t)kBvhTopFlag) {
    err.code = GLZ_E_UNSUPPORTED;
    err.msg = "more than 2^30 BVH nodes";
    return false;
  }
  // top levels of the tree for the tracers' LDS staging
  if (!d_top_.ptr && !hip_ok(d_top_.alloc(kBvhTopNodes), "alloc BVH top table", err)) return false;
  if (!hip_ok(launch_top_table(st, d_nodes_.ptr, n_nodes, d_top_.ptr), "k_top_table", err)) return false;
  dev.bvh_top = d_top_.ptr;
  dev.bvh_nodes8 = d_nodes8_.ptr;
  info.bvh_nodes8 = (uint32_t)d_nodes8_.count;
  dev.bvh_grid = out.grid;
  for (int k = 0; k < 3; ++k) {
    info.bvh_grid_lo[k] = out.grid.lo[k];
    info.bvh_grid_cell[k] = out.grid.cell[k];
  }
  dev.bvh_tris = d_tris_.ptr;
  dev.bvh_quads = d_quads_.ptr;
  // per-leaf shading records (the identity flags let k_shade skip the object->world transform exactly)
  const std::vector<uint32_t> ident = identity_flags(data.transforms);
  if (!hip_ok(d_xf_identity_.upload(ident.data(), ident.size(), st), "upload transform flags", err)) return false;
  if (!hip_ok(d_shade_tris_.alloc((size_t)n * 8), "alloc shading records", err)) return false;
  if (!hip_ok(launch_shade_records(st, n, d_tris_.ptr, d_instances_.ptr, d_indices_.ptr, d_vertices_.ptr, d_derivatives_.ptr, d_xf_identity_.ptr,
                                   d_shade_tris_.ptr), "k_shade_records", err))
    return false;
  if (!hip_ok(hipStreamSynchronize(st), "shading records", err)) return false;
  dev.shade_tris = d_shade_tris_.ptr;
  dev.xf_identity = d_xf_identity_.ptr;
  dev.n_world_tris = n;
  n_shade_slots_ = n;
  if (!build_alpha_records(err)) return false;
  info.as_levels = 1;
  info.n_as_triangles = n;
  info.as_bytes = (uint64_t)n_nodes * sizeof(BvhNode4) + (uint64_t)(n + 1) * sizeof(BvhTri) + (uint64_t)n * 128u + (uint64_t)d_quads_.count * sizeof(BvhQuad) +
                  (uint64_t)info.bvh_nodes8 * sizeof(BvhNode8);
  return true;
}

// What the alpha test of a candidate reads (DeviceScene::alpha_recs): texture coordinates and the opacity map's descriptor per triangle
// slot.  Flattened scenes only (the two-level tracer takes the material from the instance, alpha_test_instance); nothing without an
// opacity map.  Called by the flattened build and again by everything that changes a material's opacity map or moves texels.
bool Scene::build_alpha_records(Error& err) {
  dev.alpha_recs = nullptr;
  if (dev.two_level || !dev.has_non_opaque || n_shade_slots_ == 0 || !d_shade_tris_.ptr) return true;
  hipStream_t st = instance->stream;
  if (!hip_ok(d_alpha_recs_.alloc((size_t)n_shade_slots_ * 3), "alloc alpha records", err)) return false;
  if (!hip_ok(launch_alpha_records(st, n_shade_slots_, d_shade_tris_.ptr, dev.materials, dev.tex_desc, d_alpha_recs_.ptr), "k_alpha_records", err)) return false;
  if (!hip_ok(hipStreamSynchronize(st), "alpha records", err)) return false;
  dev.alpha_recs = d_alpha_recs_.ptr;
  return true;
}

bool Scene::update_textures(const glz_texture* textures, uint32_t n, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  if (n == 0 || !textures) {
    err.code = GLZ_E_ARG;
    err.msg = "the texture list must keep at least the default texture";
    return false;
  }
  std::vector<TextureData> fresh(n);
  for (uint32_t i = 0; i < n; ++i) {
    const glz_texture& t = textures[i];
    const size_t bytes = (size_t)t.width * t.height * (t.format == GLZ_TEX_GRAY ? 1 : 4);
    if (!t.pixels || !bytes || t.format < 1 || t.format > 3) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "texture has inconsistent dimensions";
      return false;
    }
    fresh[i].info = t;
    fresh[i].level0.assign(t.pixels, t.pixels + bytes);
    fresh[i].info.pixels = fresh[i].level0.data();
  }
  data.textures.swap(fresh);
  for (auto& t : data.textures) t.info.pixels = t.level0.data();
  if (!upload_textures(err)) return false;
  info.n_textures = n;
  sky_distribution_tex_ = 0xFFFFFFFFu;   // the sky map's texels may have changed: its distributions are rebuilt
  return true;
}

bool Scene::update_materials_and_lights(const glz_material* mats, uint32_t n_mats, const glz_light* lights, uint32_t n_lights,
                                        const glz_texture* textures, uint32_t n_textures, Error& err) {
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  if (n_mats != data.materials.size()) {
    err.code = GLZ_E_ARG;
    err.msg = "update_materials_and_lights: the material count must not change (meshes index materials)";
    return false;
  }
  const size_t nt = textures ? n_textures : data.textures.size();
  for (uint32_t i = 0; i < n_mats; ++i) {
    const glz_material& m = mats[i];
    if (m.diffuse >= nt || m.roughness >= nt || m.metalness >= nt || m.normal >= nt || m.opacity >= nt) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "material references a missing texture";
      return false;
    }
  }
  for (uint32_t i = 0; i < n_lights; ++i)
    if (lights[i].ltype == GLZ_LIGHT_SKY && lights[i].resource_id >= nt) {
      err.code = GLZ_E_INVALID_DATA;
      err.msg = "sky light references a missing texture";
      return false;
    }
  if (textures && !update_textures(textures, n_textures, err)) return false;
  bool opacity_changed = false;
  for (uint32_t i = 0; i < n_mats; ++i) opacity_changed |= (mats[i].opacity != 0) != (data.materials[i].opacity != 0);
  data.materials.assign(mats, mats + n_mats);
  data.lights.assign(lights, lights + n_lights);
  if (!build_materials(err)) return false;
  if (!build_lights_and_sky(err)) return false;
  if (opacity_changed) {   // the non-opaque flag lives in the leaf records; rebuilt with the instance's current options
    if (!build_bvh_as_instance_says(err)) return false;
  }
  if (!build_alpha_records(err)) return false;             // which opacity map a material names, where its texels lie
  info.n_lights = lights_no;
  info.n_rt_lights = (uint32_t)h_lights.size();
  return hip_ok(hipStreamSynchronize(instance->stream), "update_materials_and_lights", err);
}

// refresh_binded_textures (raytracer.rs:328-356): the texture array changed under the same materials and lights
bool Scene::refresh_textures(const glz_texture* textures, uint32_t n, Error& err) {
  const size_t nm = data.materials.size();
  std::vector<glz_material> mats = data.materials;
  std::vector<glz_light> lights = data.lights;
  return update_materials_and_lights(mats.data(), (uint32_t)nm, lights.data(), (uint32_t)lights.size(), textures, n, err);
}

// ---- moving instances ------------------------------------------------------------------------------------------------------------
std::vector<InstanceBoxMesh> Scene::box_meshes() const {
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  for (const TlMesh& m : tl_meshes_) ranges.emplace_back(m.index_offset, m.index_count);
  std::vector<std::vector<float>> pts = mesh_points(data, ranges);
  std::vector<InstanceBoxMesh> out(tl_meshes_.size());
  for (size_t m = 0; m < out.size(); ++m) {
    for (int k = 0; k < 3; ++k) {
      out[m].lo[k] = tl_meshes_[m].lo[k];
      out[m].hi[k] = tl_meshes_[m].hi[k];
    }
    out[m].points = std::move(pts[m]);
  }
  return out;
}

std::vector<uint32_t> Scene::instance_transforms() const {
  std::vector<uint32_t> out(h_instances.size());
  for (size_t i = 0; i < out.size(); ++i) out[i] = h_instances[i].transform_id;
  return out;
}

bool host_instance_boxes_of(const SceneData& d, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err) {
  std::vector<glz_transform> transforms = d.transforms;
  if (transforms.empty()) transforms.push_back(identity_transform());   // as Scene::create
  if (!valid_geometry(d, transforms.size(), err)) return false;
  const std::vector<RTInstance> inst = rt_instances(d);
  std::vector<uint32_t> mesh_of, transform_of(inst.size());
  const std::vector<std::pair<uint32_t, uint32_t>> ranges = unique_meshes(inst, mesh_of);
  for (size_t i = 0; i < inst.size(); ++i) transform_of[i] = inst[i].transform_id;
  std::vector<std::vector<float>> pts = mesh_points(d, ranges);
  std::vector<InstanceBoxMesh> meshes(ranges.size());
  for (size_t m = 0; m < meshes.size(); ++m) {
    InstanceBoxMesh& b = meshes[m];
    for (int k = 0; k < 3; ++k) b.lo[k] = b.hi[k] = 0.0f;
    for (size_t p = 0; p + 2 < pts[m].size(); p += 3)
      for (int k = 0; k < 3; ++k) {
        b.lo[k] = p == 0 ? pts[m][p + k] : std::min(b.lo[k], pts[m][p + k]);
        b.hi[k] = p == 0 ? pts[m][p + k] : std::max(b.hi[k], pts[m][p + k]);
      }
    b.points = std::move(pts[m]);
  }
  host_instance_boxes(mesh_of, transform_of, meshes, transforms, budget, lo, hi);
  return true;
}

// The device side of host_instance_boxes for the scene's current transforms (d_transforms_), into d_box_lo_ / d_box_hi_.
bool Scene::device_instance_boxes(uint64_t budget, Error& err) {
  hipStream_t st = instance->stream;
  const size_t nm = tl_meshes_.size(), ni = h_instances.size();
  if (!tl_points_ready_) {
    const std::vector<InstanceBoxMesh> bm = box_meshes();
    std::vector<float4> pts, mlo(nm), mhi(nm);
    tl_point_base_.assign(nm, 0);
    tl_point_count_.assign(nm, 0);
    for (size_t m = 0; m < nm; ++m) {
      tl_point_base_[m] = (uint32_t)pts.size();
      tl_point_count_[m] = bm[m].points.size() / 3;
      for (size_t p = 0; p + 2 < bm[m].points.size(); p += 3) pts.push_back(make_float4(bm[m].points[p], bm[m].points[p + 1], bm[m].points[p + 2], 0.0f));
      mlo[m] = make_float4(bm[m].lo[0], bm[m].lo[1], bm[m].lo[2], 0.0f);
      mhi[m] = make_float4(bm[m].hi[0], bm[m].hi[1], bm[m].hi[2], 0.0f);
    }
    for (size_t m = 0; m < nm; ++m)   // the corners, in host_instance_boxes' order, after every mesh's points
      for (int c = 0; c < 8; ++c)
        pts.push_back(make_float4((c & 1) ? bm[m].hi[0] : bm[m].lo[0], (c & 2) ? bm[m].hi[1] : bm[m].lo[1], (c & 4) ? bm[m].hi[2] : bm[m].lo[2], 0.0f));
    if (pts.size() >= 0xFFFFFFFFull) {
      err.code = GLZ_E_UNSUPPORTED;
      err.msg = "more than 2^32 mesh vertices";
      return false;
    }
    if (!hip_ok(d_tl_points_.upload(pts.data(), pts.size(), st), "upload mesh points", err) ||
        !hip_ok(d_tl_mesh_lo_.upload(mlo.data(), nm, st), "upload mesh boxes", err) || !hip_ok(d_tl_mesh_hi_.upload(mhi.data(), nm, st), "upload mesh boxes", err) ||
        !hip_ok(hipStreamSynchronize(st), "upload mesh points", err))
      return false;
    tl_points_ready_ = true;
  }
  // work items: an exact instance's points in chunks of one wave's share, the others' eight corners (exact_box_instances chooses, as on the host)
  constexpr uint32_t kChunk = 64u * 32u;
  const uint32_t corner_base = (uint32_t)(d_tl_points_.count - 8 * nm);
  const std::vector<uint8_t> exact = exact_box_instances(tl_mesh_of_, tl_point_count_, budget);
  std::vector<InstanceBoxItem> items;
  std::vector<uint32_t> first(ni + 1);
  for (size_t i = 0; i < ni; ++i) {
    first[i] = (uint32_t)items.size();
    const uint32_t m = tl_mesh_of_[i], t = h_instances[i].transform_id;
    if (!exact[i]) {
      items.push_back(InstanceBoxItem{t, m, corner_base + 8u * m, 8u});
      continue;
    }
    for (uint64_t p = 0; p < tl_point_count_[m]; p += kChunk)
      items.push_back(InstanceBoxItem{t, m, tl_point_base_[m] + (uint32_t)p, (uint32_t)std::min<uint64_t>(kChunk, tl_point_count_[m] - p)});
  }
  first[ni] = (uint32_t)items.size();
  DeviceBuffer<InstanceBoxItem> d_items;
  DeviceBuffer<uint32_t> d_first;
  DeviceBuffer<double> d_partial;
  if (!hip_ok(d_items.upload(items.data(), items.size(), st), "upload box items", err) || !hip_ok(d_first.upload(first.data(), first.size(), st), "upload box items", err) ||
      !hip_ok(d_partial.alloc(6 * items.size()), "alloc box partials", err))
    return false;
  if (d_box_lo_.count != ni && (!hip_ok(d_box_lo_.alloc(ni), "alloc instance boxes", err) || !hip_ok(d_box_hi_.alloc(ni), "alloc instance boxes", err))) return false;
  StreamTimer timer;
  if (!timer.start(st, err)) return false;
  if (!hip_ok(launch_instance_boxes(st, (uint32_t)items.size(), d_items.ptr, d_tl_points_.ptr, d_transforms_.ptr, d_partial.ptr, (uint32_t)ni, d_first.ptr,
                                    d_tl_mesh_lo_.ptr, d_tl_mesh_hi_.ptr, d_box_lo_.ptr, d_box_hi_.ptr), "k_instance_boxes", err))
    return false;
  timer.stop(st);
  if (!hip_ok(hipStreamSynchronize(st), "instance boxes", err)) return false;   // the staging vectors and scratch above must outlive the kernels
  box_kernel_ms = timer.ms();
  return true;
}

bool Scene::instance_boxes(bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err) {
  lo.clear();
  hi.clear();
  if (!dev.two_level) return false;
  if (!on_device) {
    host_instance_boxes(tl_mesh_of_, instance_transforms(), box_meshes(), data.transforms, budget, lo, hi);
    return true;
  }
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err) || !device_instance_boxes(budget, err)) return false;
  lo.resize(h_instances.size());
  hi.resize(h_instances.size());
  return hip_ok(hipMemcpy(lo.data(), d_box_lo_.ptr, sizeof(float4) * lo.size(), hipMemcpyDeviceToHost), "read instance boxes", err) &&
         hip_ok(hipMemcpy(hi.data(), d_box_hi_.ptr, sizeof(float4) * hi.size(), hipMemcpyDeviceToHost), "read instance boxes", err);
}

// The top level again, over the instance boxes of the current transforms; the meshes' hierarchies, leaf records and shading records
// stay where they are (their links are relative to TlasInstance::node_base / quad_base / tri_base).
bool Scene::rebuild_top_level(Error& err) {
  StreamTimer timer;
  if (!timer.start(instance->stream, err)) return false;
  if (!device_instance_boxes(kExactBoxBudget, err)) return false;
  std::vector<float4> blo, bhi;   // read back with the leaf order
  return assemble_top_level(d_box_lo_.ptr, d_box_hi_.ptr, blo, bhi, nullptr, timer, err);
}

bool Scene::update_transforms(const glz_transform* transforms, uint32_t n, Error& err) {
  if (!transforms || n != data.transforms.size()) {
    err.code = GLZ_E_ARG;
    err.msg = "update_transforms: the transform count must not change (instances index transforms)";
    return false;
  }
  if (!hip_ok(hipSetDevice(instance->device), "hipSetDevice", err)) return false;
  data.transforms.assign(transforms, transforms + n);
  const std::vector<TransformPair> xf = transform_pairs(data.transforms);
  if (!hip_ok(hipMemcpyAsync(d_transforms_.ptr, xf.data(), sizeof(TransformPair) * n, hipMemcpyHostToDevice, instance->stream), "upload transforms", err) ||
      !hip_ok(hipStreamSynchronize(instance->stream), "upload transforms", err))
    return false;
  // a flattened scene's world triangles depend on every transform: the whole structure again, with the options it was built with
  if (!dev.two_level) return build_bvh(err) && hip_ok(hipStreamSynchronize(instance->stream), "update_transforms", err);
  return rebuild_top_level(err);
}

}  // namespace glz
