// RayTraceInstance / RayTraceScene equivalents: device selection, scene upload, hierarchy build.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "device/types.h"
#include "glaze_abi.h"
#include "kernels.h"
#include "parser.h"

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
  ~Instance();
  static Instance* create(int hip_device, Error& err);
};

// ---- instance boxes of a two-level top level (scene.cpp) ----
// Past this many point transforms, the remaining instances (in instance order) take the eight corners of their mesh's box.
constexpr uint64_t kExactBoxBudget = 50000000ull;
struct InstanceBoxMesh {
  float lo[3], hi[3];          // the mesh's object box
  std::vector<float> points;   // xyz of the distinct vertices the mesh references
};
std::vector<RTInstance> rt_instances(const SceneData& d);   // the instances the device gets (dangling ones dropped)
// xyz of the distinct vertices each index range (offset, count) references, in first-use order
std::vector<std::vector<float>> mesh_points(const SceneData& d, const std::vector<std::pair<uint32_t, uint32_t>>& ranges);
// which instances take the exact box: in instance order, while the points spent stay within `budget`
std::vector<uint8_t> exact_box_instances(const std::vector<uint32_t>& mesh_of, const std::vector<uint64_t>& mesh_point_count, uint64_t budget);
// The host rule: instance i = mesh mesh_of[i] under transforms[transform_of[i]]; the f64 world AABB of the mesh's points (or of the
// corners of its box), padded for the tracer's single-precision world vertices and widened by one ulp outwards.  Non-finite
// transforms give a padded box around the origin.
void host_instance_boxes(const std::vector<uint32_t>& mesh_of, const std::vector<uint32_t>& transform_of, const std::vector<InstanceBoxMesh>& meshes,
                         const std::vector<glz_transform>& transforms, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi);
double instance_reach(const std::vector<float4>& lo, const std::vector<float4>& hi);
// The host rule on a scene description, no device: the meshes' boxes are the min / max of their vertices (a scene's own build takes
// its mesh hierarchies' root boxes).  One box per instance that names an existing mesh.
bool host_instance_boxes_of(const SceneData& d, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err);

struct StreamTimer;   // scene.cpp

// RayTraceScene (lib/src/vulkan/scene.rs:1352-1556)
class Scene {
 public:
  static Scene* create(Instance* inst, SceneData&& data, Error& err);
  // update_materials_and_lights (scene.rs:1587-1716): rebuilds RTMaterial / RTLight / sky tables.
  // The BVH is rebuilt only if a material's opacity flag changed (acceleration.rs:136-141).
  // `textures` (may be null = keep) replaces the texture array: the reference passes the raw textures for the sky
  // distributions (scene.rs:1598-1615) and re-binds the shared GPU textures separately (refresh_descriptors).
  bool update_materials_and_lights(const glz_material* mats, uint32_t n_mats, const glz_light* lights, uint32_t n_lights,
                                   const glz_texture* textures, uint32_t n_textures, Error& err);
  bool refresh_textures(const glz_texture* textures, uint32_t n, Error& err);   // refresh_binded_textures, raytracer.rs:328-356
  // New object -> world transforms, as many as the scene has (instances index them).  The structure is rebuilt with the builder, pair
  // ratio and shape the scene was created with, and equals a scene created with these transforms: a flattened scene is built again
  // in full (its world triangles depend on every transform); a two-level scene keeps its meshes' hierarchies and rebuilds the top
  // level only.  Lights, sky, materials and textures are left alone.
  bool update_transforms(const glz_transform* transforms, uint32_t n, Error& err);
  // Instance boxes of a two-level scene under its current transforms (host rule, or the device kernel); false with an empty result
  // for a flattened scene.  budget: kExactBoxBudget for the scene's own.
  bool instance_boxes(bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err);
  size_t n_tlas_records() const { return dev.two_level ? d_tlas_instances_.count : 0; }
  float box_kernel_ms = -1.0f;   // device-event time of the instance-box kernels the last time they ran (-1: never)
  // Mip levels 1.. of every texture on the device (mipchain.h: the file's levels when it brings all of them, else generated by
  // the LINEAR-blit rule, as load_texture_to_gpu does, scene.rs:1012-1263).  Built on first use: the reference's ray-tracing
  // stages only ever sample level 0, so a renderer without texture LOD never pays for them.
  bool ensure_mips(Error& err);
  bool mips_ready() const { return mips_ready_; }
  // host copy of one level of the chain (level 0 = the texture itself); empty when out of range.  Builds the chain if needed.
  bool read_mip_level(uint32_t texture, uint32_t level, std::vector<uint8_t>& pixels, uint32_t& w, uint32_t& h, Error& err);

  Instance* instance = nullptr;
  SceneData data;           // host copy (materials/lights are kept for updates)
  glz_scene_info info{};
  DeviceScene dev{};        // what the kernels see
  uint32_t lights_no = 0;   // lights.len() after reorder_lights (scene.rs:1549)
  uint32_t stack_overflow_depth = 1;

  // host mirrors of the uploaded RT arrays (debug read-back / parity with the oracle)
  std::vector<RTInstance> h_instances;
  std::vector<RTMaterial> h_materials;
  std::vector<RTLight> h_lights;
  std::vector<float> h_sky_marginal;
  struct MeshRange { uint32_t node_base, n_nodes, quad_base, tri_base; };
  std::vector<MeshRange> h_mesh_ranges;   // two-level scenes: where each mesh's nodes and leaf records sit (glz_debug_read_bvh)
  SkyHeader h_sky_header{};
  RTSky h_sky{};

 size_t d_quads_count() const { return d_quads_.count; }   // leaf records: the flattened build's, or the meshes' concatenated (glz_debug_read_bvh)
 private:
  // what shapes the acceleration structure, as the scene was built (Instance at creation; as_levels = the shape built, 1 or 2)
  struct BuildOptions {
    int builder;
    float pair_area_ratio;
    int as_levels;
  };
  BuildOptions build_opts_{};
  // two-level scenes: what the top level needs of each mesh (node, leaf and triangle bases are in h_mesh_ranges)
  struct TlMesh {
    uint32_t index_offset, index_count;
    BvhGrid grid;
    float lo[3], hi[3];   // object box (the mesh hierarchy's root box)
  };
  std::vector<TlMesh> tl_meshes_;
  // a mesh as build_two_level has just built it: what is kept of it (tl_meshes_, h_mesh_ranges) and what moves into the scene's arrays
  struct MeshBuild {
    TlMesh mesh{};
    MeshRange range{};
    DeviceBuffer<BvhNode4> nodes;
    DeviceBuffer<BvhQuad> quads;   // leaf records, object space
  };
  std::vector<uint32_t> tl_mesh_of_;   // per RTInstance
  uint32_t tl_top_nodes_ = 0;          // the top level's nodes at the head of d_nodes_
  uint32_t tl_mesh_depth_ = 0;         // deepest mesh hierarchy
  std::vector<InstanceBoxMesh> box_meshes() const;
  std::vector<uint32_t> instance_transforms() const;
  bool write_top_records(const std::vector<BvhTri>& order, double reach, Error& err);
  void finish_two_level(const HierarchyOutputs& top, float build_ms);
  bool assemble_top_level(const float4* d_lo, const float4* d_hi, std::vector<float4>& h_lo, std::vector<float4>& h_hi, const std::vector<MeshBuild>* built,
                          StreamTimer& timer, Error& err);
  bool rebuild_top_level(Error& err);
  bool device_instance_boxes(uint64_t budget, Error& err);   // -> d_box_lo_ / d_box_hi_
  // the device side of the instance boxes, built on the first update: the meshes' distinct vertices then eight corners per mesh
  bool tl_points_ready_ = false;
  std::vector<uint64_t> tl_point_count_;
  std::vector<uint32_t> tl_point_base_;
  DeviceBuffer<float4> d_tl_points_, d_tl_mesh_lo_, d_tl_mesh_hi_, d_box_lo_, d_box_hi_;

  bool upload_geometry(Error& err);
  bool upload_textures(Error& err);
  bool update_textures(const glz_texture* textures, uint32_t n, Error& err);
  bool build_materials(Error& err);
  bool build_lights_and_sky(Error& err);
  bool build_bvh(Error& err);
  bool build_bvh_as_instance_says(Error& err);
  bool build_alpha_records(Error& err);   // DeviceScene::alpha_recs, after anything that changes materials, textures or the triangle slots
  bool build_two_level(Error& err);

  DeviceBuffer<float4> d_vertices_, d_derivatives_;
  DeviceBuffer<uint32_t> d_indices_, d_inst_base_;
  DeviceBuffer<RTInstance> d_instances_;
  DeviceBuffer<RTMaterial> d_materials_;
  DeviceBuffer<RTLight> d_lights_;
  DeviceBuffer<TransformPair> d_transforms_;
  DeviceBuffer<TexDesc> d_tex_desc_, d_tex_mip_desc_;
  DeviceBuffer<uint8_t> d_tex_pool_, d_tex_mip_pool_;
  DeviceBuffer<uint32_t> d_tex_mip_base_;
  bool mips_ready_ = false;
  std::vector<std::vector<std::vector<uint8_t>>> h_mips_;   // [texture][level - 1] pixels (host copy for read_mip_level)
  DeviceBuffer<float> d_srgb_lut_, d_sky_marginal_, d_sky_cond_values_, d_sky_cond_cdf_;
  DeviceBuffer<BvhNode4> d_nodes_, d_top_;
  DeviceBuffer<BvhTri> d_tris_;
  DeviceBuffer<BvhQuad> d_quads_;   // flattened build: per-leaf records of the tracer (built by build_hierarchy)
  DeviceBuffer<BvhNode8> d_nodes8_;   // flattened build: the hierarchy eight wide (k_trace8)
  DeviceBuffer<float4> d_shade_tris_;
  DeviceBuffer<float4> d_alpha_recs_;   // DeviceScene::alpha_recs
  uint32_t n_shade_slots_ = 0;          // triangle slots of the flattened build (records in d_shade_tris_)
  DeviceBuffer<uint32_t> d_xf_identity_;
  DeviceBuffer<TlasInstance> d_tlas_instances_;
  std::vector<uint32_t> inst_base_;
  uint32_t sky_distribution_tex_ = 0xFFFFFFFFu;
};

bool hip_ok(hipError_t e, const char* what, Error& err);

}  // namespace glz
