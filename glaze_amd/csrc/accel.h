// The acceleration structure of a scene in both its shapes -- one hierarchy over every instanced triangle (flattened), or one per
// mesh under a top level over the instances (two levels) -- with its update paths.  It owns everything it builds; what it builds
// FROM (the geometry, the material table, the texture descriptors) belongs to the scene and comes in as a Sources with every call.
#pragma once
#include <vector>

#include "hip_util.h"
#include "instance_boxes.h"
#include "kernels.h"
#include "parser.h"
#include "shading_tables.h"
#include "textures.h"

namespace glz {

// The geometry as Scene uploads it: the device arrays the kernels and the builds read, and the host side of the instances
struct Geometry {
  DeviceBuffer<float4> vertices, derivatives;
  DeviceBuffer<uint32_t> indices, inst_base;
  DeviceBuffer<RTInstance> instances;
  DeviceBuffer<TransformPair> transforms;
  DeviceBuffer<float> srgb_lut;
  std::vector<RTInstance> h_instances;   // host mirror of `instances` (debug read-back / parity with the oracle)
  std::vector<uint32_t> h_inst_base;     // first world triangle of each instance
  uint64_t n_world_triangles = 0;
};

// what Geometry::transforms holds: object -> world as given, world -> object inverted in double precision (identity when singular or not finite)
std::vector<TransformPair> transform_pairs(const std::vector<glz_transform>& transforms);

class Accel {
 public:
  struct Sources {
    hipStream_t stream;
    const SceneData& data;   // transforms; vertices and indices for the instance boxes
    const Geometry& geometry;
    const ShadingTables& tables;
    const Textures& textures;
  };
  // what shapes the structure (as_levels: 0 = automatic, 1 = flattened, 2 = two levels; Instance holds the meaning of the others)
  struct BuildOptions {
    int builder;
    float pair_area_ratio;
    int as_levels;
  };
  // The structure with these options; from then on they are the scene's own (with as_levels = the shape built) and rebuild() keeps them
  bool build(const BuildOptions& opts, const Sources& s, Error& err);
  // After new transforms: a flattened scene is built again in full (its world triangles depend on every transform), a two-level scene
  // keeps its meshes' hierarchies, leaf records and shading records and gets a new top level.
  bool rebuild(const Sources& s, Error& err);
  // New vertices in [first, first + count) of the vertex buffer, already on the device with their derivatives (Scene::update_vertices).
  // GLZ_GEOMETRY_REBUILD runs the builder again with the options and the shape the scene has.  GLZ_GEOMETRY_REFIT keeps the topology:
  // leaf records and leaf boxes again from the vertices, the wide nodes' boxes fitted level by level, the grid re-derived from the root
  // box and every child box quantised on it (kernels_refit.hip) -- for a flattened scene over the whole structure, for a two-level
  // scene per mesh whose indices reach into the range, each in its object space, and then the top level as rebuild() makes it.
  // timer: started by the caller where glz_geometry_update_info::update_ms (and info.build_ms) is to begin.
  bool update_geometry(const Sources& s, int mode, uint32_t first, uint32_t count, StreamTimer& timer, Error& err);
  // What a refit needs of the structure as it stands, made on the first refit after a build and kept until the next build: the refit plan
  // (RefitPlan) and the box-area figure of the structure as built -- so it runs BEFORE the new vertices go in.  Nothing when it is there.
  bool prepare_refit(const Sources& s, Error& err);
  // What the last update_geometry did; GLZ_E_ARG before any.  The box-area figures come from the refit plans: after a rebuild there is
  // none yet, and it is made here, on request, so that a caller who rebuilds every frame and never asks does not pay for it.
  bool geometry_update(const Sources& s, glz_geometry_update_info& out, Error& err);
  // What the alpha test of a candidate reads (DeviceScene::alpha_recs): texture coordinates and the opacity map's descriptor per triangle
  // slot.  Flattened scenes only (the two-level tracer takes the material from the instance, alpha_test_instance); nothing without an
  // opacity map.  Called by the flattened build and again after everything that changes a material's opacity map or moves texels.
  bool build_alpha_records(const Sources& s, Error& err);
  // Instance boxes of a two-level scene under its current transforms (host rule, or the device kernel); false with an empty result
  // for a flattened scene.
  bool instance_boxes(const Sources& s, bool on_device, uint64_t budget, std::vector<float4>& lo, std::vector<float4>& hi, Error& err);

  bool two_level() const { return two_level_; }
  size_t n_tlas_records() const { return two_level_ ? d_tlas_instances_.count : 0; }
  size_t n_leaf_records() const { return d_quads_.count; }   // the flattened build's, or the meshes' concatenated (glz_debug_read_bvh)
  void describe(DeviceScene& dev) const;       // bvh_*, shade_tris, alpha_recs, tlas_*, xf_identity, two_level, n_world_tris
  void describe(glz_scene_info& info) const;   // bvh_*, bounds_*, build_ms, as_*, n_as_triangles

  uint32_t stack_overflow_depth = 1;
  float box_kernel_ms = -1.0f;   // device-event time of the instance-box kernels the last time they ran (-1: never)
  struct MeshRange { uint32_t node_base, n_nodes, quad_base, tri_base; };
  std::vector<MeshRange> h_mesh_ranges;   // two-level scenes: where each mesh's nodes and leaf records sit (glz_debug_read_bvh)

 private:
  // two-level scenes: what the top level needs of each mesh (node, leaf and triangle bases are in h_mesh_ranges)
  struct TlMesh {
    uint32_t index_offset, index_count;
    BvhGrid grid;
    float lo[3], hi[3];   // object box (the mesh hierarchy's root box)
  };
  // a mesh as build_two_level has just built it: what is kept of it (tl_meshes_, h_mesh_ranges) and what moves into the scene's arrays
  struct MeshBuild {
    TlMesh mesh{};
    MeshRange range{};
    DeviceBuffer<BvhNode4> nodes;
    DeviceBuffer<BvhQuad> quads;   // leaf records, object space
  };
  // The refit plan of one hierarchy (the flattened scene's, or one mesh's): its wide nodes grouped by height above the leaves for the
  // level launches, and a float box per leaf and per node.  Links are relative to the hierarchy's first node and first leaf record, so a
  // mesh's plan outlives a new top level.  Not counted in as_bytes: 32 bytes per leaf, 36 per 4-wide and per 8-wide node.
  struct RefitPlan {
    uint32_t n_leaves = 0;
    DeviceBuffer<uint32_t> order4, order8;
    std::vector<uint32_t> first4, first8;   // level offsets into order4 / order8 (height 0 first)
    DeviceBuffer<float4> leaf_lo, leaf_hi, lo4, hi4, lo8, hi8;
    float area_built = 0.0f, area = 0.0f;   // glz_geometry_update_info::box_area_built / box_area, this hierarchy's share
  };
  // where a plan's hierarchy lies and what its leaves are made from
  struct RefitTarget {
    BvhNode4* nodes;
    uint32_t n_nodes;
    BvhNode8* nodes8;
    uint32_t n_nodes8;
    BvhQuad* quads;
    BvhTri* tris;
    const RTInstance* instances;
    const TransformPair* transforms;
  };
  struct RefitResult {
    BvhGrid grid;
    float4 lo, hi;   // the root box
  };
  RefitTarget refit_target(const Sources& s, size_t plan) const;
  bool make_plan(hipStream_t st, const RefitTarget& t, uint32_t n_leaves, RefitPlan& p, Error& err);
  bool refit(hipStream_t st, const Sources& s, const RefitTarget& t, RefitPlan& p, bool write, RefitResult& out, Error& err);
  bool offsets_fit(Error& err) const;   // kernels.h traversal_offsets_exceeded for what has been built: GLZ_E_INVALID_DATA
  bool build_bvh(const Sources& s, Error& err);
  bool build_two_level(const Sources& s, Error& err);
  bool assemble_top_level(const Sources& s, const float4* d_lo, const float4* d_hi, std::vector<float4>& h_lo, std::vector<float4>& h_hi,
                          const std::vector<MeshBuild>* built, StreamTimer& timer, Error& err);
  bool write_top_records(const Sources& s, const std::vector<BvhTri>& order, double reach, Error& err);
  void finish_two_level(const Sources& s, const HierarchyOutputs& top, float build_ms);
  bool device_instance_boxes(const Sources& s, uint64_t budget, Error& err);   // -> d_box_lo_ / d_box_hi_
  std::vector<InstanceBoxMesh> box_meshes(const SceneData& data) const;

  BuildOptions build_opts_{};
  bool two_level_ = false;
  bool alpha_ready_ = false;      // d_alpha_recs_ belongs to the structure, the materials and the texels as they are
  uint32_t n_world_tris_ = 0;     // DeviceScene::n_world_tris: the world count in both shapes
  uint32_t n_shade_slots_ = 0;    // triangle slots of the flattened build (records in d_shade_tris_)
  BvhGrid grid_{};
  glz_scene_info info_{};         // the fields describe(glz_scene_info&) copies
  std::vector<TlMesh> tl_meshes_;
  std::vector<uint32_t> tl_mesh_of_;   // per RTInstance
  uint32_t tl_top_nodes_ = 0;          // the top level's nodes at the head of d_nodes_
  uint32_t tl_mesh_depth_ = 0;         // deepest mesh hierarchy
  // the device side of the instance boxes, built on the first update: the meshes' distinct vertices then eight corners per mesh
  bool tl_points_ready_ = false;
  std::vector<uint64_t> tl_point_count_;
  std::vector<uint32_t> tl_point_base_;
  DeviceBuffer<float4> d_tl_points_, d_tl_mesh_lo_, d_tl_mesh_hi_, d_box_lo_, d_box_hi_;

  // refit: one plan (flattened) or one per mesh; empty = none for the structure as it is.  Two levels: the meshes' pseudo-instances,
  // the identity transform and its flag as their builds had them, and the lowest / highest vertex index each mesh references.
  std::vector<RefitPlan> plans_;
  DeviceBuffer<RTInstance> d_tl_pseudo_;
  DeviceBuffer<TransformPair> d_tl_ident_;
  DeviceBuffer<uint32_t> d_tl_one_;
  std::vector<std::pair<uint32_t, uint32_t>> tl_vertex_span_;
  DeviceBuffer<BvhGrid> d_refit_grid_;
  DeviceBuffer<float> d_refit_area_;
  glz_geometry_update_info update_{};
  bool update_valid_ = false;

  DeviceBuffer<BvhNode4> d_nodes_, d_top_;
  DeviceBuffer<BvhTri> d_tris_;
  DeviceBuffer<BvhQuad> d_quads_;     // per-leaf records of the tracer (built by build_hierarchy)
  DeviceBuffer<BvhNode8> d_nodes8_;   // flattened build: the hierarchy eight wide (k_trace8)
  DeviceBuffer<float4> d_shade_tris_;
  DeviceBuffer<float4> d_alpha_recs_;   // DeviceScene::alpha_recs
  DeviceBuffer<uint32_t> d_xf_identity_;
  DeviceBuffer<TlasInstance> d_tlas_instances_;
};

}  // namespace glz
