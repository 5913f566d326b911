// RayTraceInstance / RayTraceScene equivalents: device selection, scene upload, and the parts a scene is made of -- the textures
// (textures.h), the shading tables (shading_tables.h) and the acceleration structure (accel.h).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "accel.h"
#include "device/types.h"
#include "glaze_abi.h"
#include "hip_util.h"
#include "instance_boxes.h"
#include "kernels.h"
#include "parser.h"
#include "shading_tables.h"
#include "textures.h"

namespace glz {

// RayTraceInstance (lib/src/vulkan/instance.rs:376-427): one HIP device + the stream all work runs on.
struct Instance {
  int device = -1;
  hipStream_t stream = nullptr;
  std::string arch;
  // two triangles share a leaf when area(joint box) <= ratio * (area(a) + area(b)); tuning switch GLAZE_BVH_PAIRS=<ratio>, 0 = never
  float bvh_pair_area_ratio = getenv("GLAZE_BVH_PAIRS") ? (float)atof(getenv("GLAZE_BVH_PAIRS")) : kPairAreaRatio;
  int bvh_builder = 3;   // kBvhBuilder* for scenes created afterwards (glz_instance_set_bvh_builder); 3 = kBvhBuilderAuto
  // acceleration-structure shape for scenes created afterwards (glz_instance_set_as_levels): 0 = automatic (two levels when the
  // instances hold more than four times the triangles of the meshes they share), 1 = always flattened, 2 = always two levels
  int as_levels = getenv("GLAZE_AS_LEVELS") ? atoi(getenv("GLAZE_AS_LEVELS")) : 0;
  // everything that shapes the acceleration structure of scenes built on this instance (replicas on other GPUs must match)
  void copy_build_options(const Instance& o) {
    bvh_pair_area_ratio = o.bvh_pair_area_ratio;
    bvh_builder = o.bvh_builder;
    as_levels = o.as_levels;
  }
  Accel::BuildOptions build_options() const { return Accel::BuildOptions{bvh_builder, bvh_pair_area_ratio, as_levels}; }
  ~Instance();
  static Instance* create(int hip_device, Error& err);
};

// RayTraceScene (lib/src/vulkan/scene.rs:1352-1556)
class Scene {
 public:
  static Scene* create(Instance* inst, SceneData&& data, Error& err);
  // update_materials_and_lights (scene.rs:1587-1716): rebuilds RTMaterial / RTLight / sky tables.
  // The BVH is rebuilt only if a material's opacity flag changed (acceleration.rs:136-141), with the instance's current options.
  // `textures` (may be null = keep) replaces the texture array: the reference passes the raw textures for the sky
  // distributions (scene.rs:1598-1615) and re-binds the shared GPU textures separately (refresh_descriptors).
  bool update_materials_and_lights(const glz_material* mats, uint32_t n_mats, const glz_light* lights, uint32_t n_lights,
                                   const glz_texture* textures, uint32_t n_textures, Error& err);
  bool refresh_textures(const glz_texture* textures, uint32_t n, Error& err);   // refresh_binded_textures, raytracer.rs:328-356
  // New object -> world transforms, as many as the scene has (instances index them).  The structure is rebuilt with the builder, pair
  // ratio and shape the scene was created with, and equals a scene created with these transforms (Accel::rebuild).  Lights, sky,
  // materials and textures are left alone.
  bool update_transforms(const glz_transform* transforms, uint32_t n, Error& err);
  // New vertices (positions, normals, texture coordinates) for [first, first + n) of the vertex buffer; indices and everything else stay.
  // The derivatives are computed again and the structure follows by Accel::update_geometry in `mode` (GLZ_GEOMETRY_*); either way the
  // scene traces and renders as one created with the new vertices does.  Refused arguments (GLZ_E_ARG) leave the scene untouched.
  bool update_vertices(const glz_vertex* vertices, uint32_t first, uint32_t n, int mode, Error& err);
  bool geometry_update_info(glz_geometry_update_info& out, Error& err);   // Accel::geometry_update
  // Instance boxes of a two-level scene under its current transforms (host rule, or the device kernel); false with an empty result
  // for a flattened scene.  budget: kExactBoxBudget for the scene's own.
  bool instance_boxes(bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err);
  // Mip levels 1.. of every texture on the device.  Built on first use: the reference's ray-tracing stages only ever sample
  // level 0, so a renderer without texture LOD never pays for them.
  bool ensure_mips(Error& err);
  bool mips_ready() const { return textures_.mips_ready(); }
  // host copy of one level of the chain (level 0 = the texture itself); empty when out of range.  Builds the chain if needed.
  bool read_mip_level(uint32_t texture, uint32_t level, std::vector<uint8_t>& pixels, uint32_t& w, uint32_t& h, Error& err);
  const ShadingTables& tables() const { return tables_; }
  const Accel& accel() const { return accel_; }

  Instance* instance = nullptr;
  SceneData data;           // host copy (materials/lights are kept for updates)
  glz_scene_info info{};
  // What the kernels see; every launch copies it.  Written by compose() alone, from the parts as they are, at the end of everything
  // that changes one of them -- on failure too, so that it names live buffers or null, never freed memory.
  DeviceScene dev{};

 private:
  struct Composed;   // scope guard: compose() on every way out
  void compose();
  bool upload_geometry(Error& err);
  Accel::Sources sources() const { return Accel::Sources{instance->stream, data, geometry_, tables_, textures_}; }

  Geometry geometry_;
  Textures textures_;
  ShadingTables tables_;
  Accel accel_;
};

}  // namespace glz
