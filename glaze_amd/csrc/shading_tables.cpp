// Material, light and sky tables (shading_tables.h).
#include "shading_tables.h"

#include <cmath>
#include <cstring>
#include <utility>

#include "host_math.h"
#include "instance_boxes.h"

namespace glz {

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

bool metal_spectra(uint32_t metal, float* ior_out, float* ior2abs2_out) {
  if (metal >= GLZ_METAL_COUNT) return false;
  for (int i = 0; i < 16; ++i) {
    const float n = GLZ_METAL_N[metal][i], k = GLZ_METAL_K[metal][i];
    ior_out[i] = n;
    ior2abs2_out[i] = (n * n) + (k * k);
  }
  return true;
}

bool conductor_finite(const float* ior, const float* ior2abs2) {
  const double big = 1152921504606846976.0;   // 2^60
  for (int i = 0; i < 16; ++i) {
    const double n = ior[i], a = ior2abs2[i];
    if (!std::isfinite(n) || !std::isfinite(a) || std::fabs(n) > big || std::fabs(a) > big) return false;
    const double need = (std::fabs(a) + 4.0 * std::fabs(n) + 5.0) / 1024.0;
    // a + 2nc + c^2 on [-2, 2]: the ends, and the vertex c = -n where it lies inside
    double lo = std::fmin(a + 4.0 * n + 4.0, a - 4.0 * n + 4.0);
    if (std::fabs(n) <= 2.0) lo = std::fmin(lo, a - n * n);
    if (!(lo >= need)) return false;
    // a c^2 + 2nc + 1: the ends, and the vertex c = -n / a (for a < 0 the maximum, which lowers nothing)
    lo = std::fmin(4.0 * a + 4.0 * n + 1.0, 4.0 * a - 4.0 * n + 1.0);
    if (a != 0.0 && std::fabs(n) <= 2.0 * std::fabs(a)) lo = std::fmin(lo, 1.0 - n * n / a);
    if (!(lo >= need)) return false;
  }
  return true;
}

// load_raytrace_materials_to_gpu (scene.rs:1821-1860)
bool ShadingTables::build_materials(hipStream_t st, const std::vector<glz_material>& materials, Error& err) {
  h_materials.clear();
  for (const glz_material& m : materials) {
    RTMaterial r{};
    for (int i = 0; i < 3; ++i) {
      r.diffuse_mul[i] = (float)m.diffuse_mul[i] / 255.0f;   // col_int_to_f32, scene.rs:1930-1937
      r.emissive_col[i] = m.has_emissive ? (float)m.emissive_col[i] / 255.0f : 0.0f;
    }
    r.diffuse_mul[3] = r.emissive_col[3] = 1.0f;
    metal_spectra(m.metal < GLZ_METAL_COUNT ? m.metal : 0, r.metal_ior.w, r.metal_fresnel.w);
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
  return upload_materials(st, err);
}

bool ShadingTables::debug_set_spectra(hipStream_t st, uint32_t material, const float* ior, const float* ior2abs2, Error& err) {
  if (material >= h_materials.size()) return err.fail(GLZ_E_ARG, "no such material");
  memcpy(h_materials[material].metal_ior.w, ior, 64);
  memcpy(h_materials[material].metal_fresnel.w, ior2abs2, 64);
  return upload_materials(st, err);
}

bool ShadingTables::upload_materials(hipStream_t st, Error& err) {
  // the tables the shading kernels read at every hit, derived from the records just made (device/types.h): MatCompact, and the spectra
  // on their own, each distinct pair once; a material's index word says whether its pair is conductor_finite
  h_mat_compact.clear();
  h_metal_spectra.clear();
  std::vector<uint32_t> finite;   // per distinct pair: kSpectraConductorFinite or 0
  for (const RTMaterial& r : h_materials) {
    MetalSpectra sp;
    sp.ior = r.metal_ior;
    sp.fresnel = r.metal_fresnel;
    size_t slot = 0;
    while (slot < h_metal_spectra.size() && memcmp(&h_metal_spectra[slot], &sp, sizeof(sp)) != 0) ++slot;
    if (slot == h_metal_spectra.size()) {
      h_metal_spectra.push_back(sp);
      finite.push_back(conductor_finite(sp.ior.w, sp.fresnel.w) ? kSpectraConductorFinite : 0u);
    }
    h_mat_compact.push_back(compact_material(r, (uint32_t)slot | finite[slot]));
  }
  // The three device arrays belong together (MatCompact::spectra indexes the spectra table, both mirror the RTMaterial array): they are
  // uploaded into new buffers and take the old ones' place only when all three are there, so a failed upload leaves the device with the
  // consistent set it had.
  DeviceBuffer<RTMaterial> materials_new;
  DeviceBuffer<MetalSpectra> spectra_new;
  DeviceBuffer<MatCompact> compact_new;
  if (!hip_ok(materials_new.upload(h_materials.data(), h_materials.size(), st), "upload materials", err)) return false;
  if (!hip_ok(spectra_new.upload(h_metal_spectra.data(), h_metal_spectra.size(), st), "upload metal spectra", err)) return false;
  if (!hip_ok(compact_new.upload(h_mat_compact.data(), h_mat_compact.size(), st), "upload compact materials", err)) return false;
  if (!hip_ok(hipStreamSynchronize(st), "materials upload", err)) return false;
  d_materials_ = std::move(materials_new);
  d_metal_spectra_ = std::move(spectra_new);
  d_mat_compact_ = std::move(compact_new);
  return true;
}

void sky_row_pairs(const float* marginal_values, const float* conditional_integrals, size_t n, float* pairs_out) {
  for (size_t y = 0; y < n; ++y) {
    pairs_out[2 * y] = marginal_values[y];
    pairs_out[2 * y + 1] = conditional_integrals[y];
  }
}

float sky_cdf_search(const float* cdf, uint32_t size_u, float xi, const uint16_t* bracket, uint32_t* offset_out) {
  const int size = (int)size_u;
  int first = 0, len = size;
  if (bracket != nullptr && xi >= 0.0f && xi < 1.0f) {
    const int b = (int)(xi * (float)kSkyBracketBuckets);
    const int lo = (int)bracket[b], hi = (int)bracket[b + 1];
    if (lo != (int)kSkyBracketFallback) {
      first = lo;
      len = hi - lo;
    }
  }
  while (len > 0) {
    const int half = len >> 1, middle = first + half;
    if (cdf[middle] <= xi) {
      first = middle + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  int off = first - 1;
  off = off < 0 ? 0 : (off > size - 2 ? size - 2 : off);
  const float cur = cdf[off], next = cdf[off + 1];
  float du = xi - cur;
  if (next - cur > 0.0f) du /= next - cur;
  *offset_out = (uint32_t)off;
  return ((float)off + du) / (float)size;
}

void sky_bracket_table(const float* cdf, uint32_t size, uint16_t* table_out) {
  bool monotone = size < kSkyBracketFallback;
  for (uint32_t i = 0; monotone && i + 1 < size; ++i) monotone = cdf[i + 1] >= cdf[i];   // (a NaN fails it)
  if (monotone && size != 0u) monotone = cdf[0] == cdf[0];   // (a cdf of one entry that is a NaN)
  for (uint32_t b = 0; b <= kSkyBracketBuckets; ++b) {
    if (!monotone) {
      table_out[b] = (uint16_t)kSkyBracketFallback;
      continue;
    }
    const float xi = (float)b / (float)kSkyBracketBuckets;
    int first = 0, len = (int)size;   // the full search's bisection
    while (len > 0) {
      const int half = len >> 1, middle = first + half;
      if (cdf[middle] <= xi) {
        first = middle + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    table_out[b] = (uint16_t)first;
  }
}

bool ShadingTables::has_non_opaque() const {
  for (const RTMaterial& m : h_materials)
    if (m.opacity != 0u) return true;
  return false;
}

// reorder_lights (scene.rs:628-635), load_raytrace_lights_to_gpu (:1863-1927),
// calculate_skymap_distributions + build_sky_raytrace_buffers (:2191-2313)
bool ShadingTables::build_lights_and_sky(hipStream_t st, const SceneData& data, size_t n_instances, Error& err) {
  std::vector<glz_light> ordered;
  const glz_light* sky = nullptr;
  for (const glz_light& l : data.lights) {
    if (l.ltype > GLZ_LIGHT_SKY) return err.fail(GLZ_E_INVALID_DATA, "Invalid enum value for LightType");
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
        if (id >= n_instances) return err.fail(GLZ_E_INVALID_DATA, "area light refers to a missing instance");
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

  // sky: Light::default() when the scene has none (scene.rs:2249)
  glz_light dflt{};
  dflt.intensity = 1.0f;
  const glz_light& sl = has_sky ? ordered.back() : dflt;
  if (sl.resource_id >= data.textures.size()) return err.fail(GLZ_E_INVALID_DATA, "sky light references a missing texture");
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
    // what a sample reads besides the row search, where it costs no scattered load: the conditional tables' first words in the header
    // (the kernel arguments), the row's two entries of h_sky_marginal as one pair
    h_sky_header.cond_cdf00 = cond_cdf.empty() ? 0.0f : cond_cdf[0];
    h_sky_header.cond_value00 = values.empty() ? 0.0f : values[0];
    h_sky_rows.resize(2 * (size_t)H);
    sky_row_pairs(h_sky_marginal.data() + h_sky_header.marginal_cdf_count, h_sky_marginal.data() + h_sky_header.conditional_integral_offset, H, h_sky_rows.data());
    if (!hip_ok(d_sky_rows_.upload(reinterpret_cast<const float2*>(h_sky_rows.data()), H, st), "upload sky rows", err)) return false;
    // the marginal cdf's bracket table travels behind the three arrays, in the same buffer (sky_bracket_offset: whole 16-byte pieces)
    h_sky_bracket.assign(kSkyBracketFloats * 2u, 0);
    sky_bracket_table(h_sky_marginal.data(), h_sky_header.marginal_cdf_count, h_sky_bracket.data());
    std::vector<float> with_bracket(sky_bracket_offset(h_sky_header.marginal_cdf_count) + kSkyBracketFloats, 0.0f);
    memcpy(with_bracket.data(), h_sky_marginal.data(), h_sky_marginal.size() * sizeof(float));
    memcpy(with_bracket.data() + sky_bracket_offset(h_sky_header.marginal_cdf_count), h_sky_bracket.data(), h_sky_bracket.size() * sizeof(uint16_t));
    if (!hip_ok(d_sky_marginal_.upload(with_bracket.data(), with_bracket.size(), st), "upload sky marginal", err)) return false;
    if (!hip_ok(d_sky_cond_values_.upload(values.data(), values.size(), st), "upload sky values", err)) return false;
    if (!hip_ok(d_sky_cond_cdf_.upload(cond_cdf.data(), cond_cdf.size(), st), "upload sky cdf", err)) return false;
    if (!hip_ok(hipStreamSynchronize(st), "sky upload", err)) return false;
    sky_w_ = W;
    sky_h_ = H;
    sky_distribution_tex_ = h_sky.tex_id;
  }
  return hip_ok(hipStreamSynchronize(st), "lights upload", err);
}

void ShadingTables::describe(DeviceScene& dev) const {
  dev.materials = d_materials_.ptr;
  dev.mat_compact = d_mat_compact_.ptr;
  dev.metal_spectra = d_metal_spectra_.ptr;
  dev.n_metal_spectra = (uint32_t)d_metal_spectra_.count;
  dev.n_materials = (uint32_t)d_materials_.count;
  dev.has_non_opaque = has_non_opaque() ? 1u : 0u;
  dev.lights = d_lights_.ptr;
  dev.n_rt_lights = (uint32_t)d_lights_.count;   // (the records on the device, whatever a failed update left in h_lights)
  dev.sky = h_sky;
  dev.sky_header = h_sky_header;
  dev.sky_marginal = d_sky_marginal_.ptr;
  dev.sky_cdf = d_sky_marginal_.ptr;   // (k_shade points its copy at an LDS copy of the same entries)
  dev.sky_rows = d_sky_rows_.ptr;
  dev.sky_cond_values = d_sky_cond_values_.ptr;
  dev.sky_cond_cdf = d_sky_cond_cdf_.ptr;
  dev.sky_w = sky_w_;
  dev.sky_h = sky_h_;
}

}  // namespace glz
