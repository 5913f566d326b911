// RayTraceInstance / RayTraceScene equivalents: device selection, scene upload, and the parts a scene is made of -- the textures
// (textures.h), the shading tables (shading_tables.h), the acceleration structure (accel.h) and the vertex deformers (deformers.h).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "accel.h"
#include "deformers.h"
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
  // glz_debug_scene_set_spectra: metal spectra of the caller's for one material, for the debug BSDF hooks (ShadingTables::debug_set_spectra)
  bool debug_set_spectra(uint32_t material, const float* ior, const float* ior2abs2, Error& err);
  // New object -> world transforms, as many as the scene has (instances index them).  The structure is rebuilt with the builder, pair
  // ratio and shape the scene was created with, and equals a scene created with these transforms (Accel::rebuild).  Lights, sky,
  // materials and textures are left alone.
  bool update_transforms(const glz_transform* transforms, uint32_t n, Error& err);
  // New vertices (positions, normals, texture coordinates) for [first, first + n) of the vertex buffer; indices and everything else stay.
  // The derivatives are computed again and the structure follows by Accel::update_geometry in `mode` (GLZ_GEOMETRY_*); either way the
  // scene traces and renders as one created with the new vertices does.  Refused arguments (GLZ_E_ARG) leave the scene untouched.
  bool update_vertices(const glz_vertex* vertices, uint32_t first, uint32_t n, int mode, Error& err);
  bool geometry_update_info(glz_geometry_update_info& out, Error& err);   // Accel::geometry_update
  // ---- skins, morph targets and normal sets: the scene's Deformers part (deformers.h describes every call) ----
  int add_skin(const glz_skin& skin, Error& err) { return deformers_.add_skin(deformer_sources(), skin, err); }
  bool remove_skin(int id, Error& err) { return deformers_.remove_skin(id, err); }
  bool set_skin_blend(int id, int blend, Error& err) { return deformers_.set_skin_blend(id, blend, err); }
  int skin_blend(int id, Error& err) const { return deformers_.skin_blend(id, err); }
  int add_morph(const glz_morph& morph, Error& err) { return deformers_.add_morph(deformer_sources(), morph, err); }
  bool remove_morph(int id, Error& err) { return deformers_.remove_morph(id, err); }
  bool remove_normals(int id, Error& err) { return deformers_.remove_normals(id, err); }
  int add_skeleton(const glz_skeleton& skeleton, Error& err) { return deformers_.add_skeleton(deformer_sources(), skeleton, err); }
  bool remove_skeleton(int id, Error& err) { return deformers_.remove_skeleton(id, err); }
  int add_clip(const glz_clip& clip, Error& err) { return deformers_.add_clip(deformer_sources(), clip, err); }
  bool remove_clip(int id, Error& err) { return deformers_.remove_clip(id, err); }
  bool played_span(const glz_play* plays, uint32_t n, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
    return deformers_.played_span(plays, n, who, first, count, err);
  }
  bool clip_bones(const glz_play& play, float* rows_out, float* weights_out, Error& err) const { return deformers_.clip_bones(deformer_sources(), play, rows_out, weights_out, err); }
  bool time_clip(const glz_play* plays, uint32_t n, uint32_t reps, float* kernel_ms, Error& err) const { return deformers_.time_clip(deformer_sources(), plays, n, reps, kernel_ms, err); }
  bool animated_span(const glz_animation* anim, const char* who, uint32_t& first, uint32_t& count, Error& err) const {
    return deformers_.animated_span(anim, who, first, count, err);
  }
  bool animate_into(const glz_animation& anim, float4* span, uint32_t span_first, Deformers::AnimationUploads& up, hipStream_t st, Error& err) const {
    return deformers_.animate_into(anim, span, span_first, up, st, err);
  }
  bool time_skin(const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const { return deformers_.time_skin(deformer_sources(), pose, reps, kernel_ms, err); }
  bool time_morph(const glz_animation& one, uint32_t reps, float* kernel_ms, uint64_t* bytes, Error& err) const {
    return deformers_.time_morph(deformer_sources(), one, reps, kernel_ms, bytes, err);
  }
  bool time_normals(int id, uint32_t reps, float ms[2], uint64_t bytes[2], Error& err) const { return deformers_.time_normals(deformer_sources(), id, reps, ms, bytes, err); }
  // everything that makes `src`'s skins, morphs and normal sets, on this scene (a replica on another device, made of src's current vertices)
  bool copy_deformers(const Scene& src, Error& err) { return deformers_.copy_from(deformer_sources(), src.deformers_, err); }
  // Morphs and poses in one update of the structure (glz_renderer_animate): the animation's kernels into the vertex buffer
  // (Deformers::animate_into), then what update_vertices does after its upload, over the span from the lowest to the highest vertex
  // written.  The host mirror (data.vertices) is NOT written: the span is marked stale and read back when a reader asks (host_data()).
  bool animate(const glz_animation& anim, int mode, Error& err) { return run_animation(anim, mode, "animate", err); }
  // animate with no morph named
  bool pose_skins(const glz_pose* poses, uint32_t n_poses, int mode, Error& err) { return run_animation(glz_animation{nullptr, 0, poses, n_poses}, mode, "pose_skins", err); }
  // Clips played in one update of the structure (glz_renderer_play): k_clip_bones and the skins' kernels into the vertex buffer
  // (Deformers::play_into), then the same tail as animate, over the span from the lowest to the highest vertex written.
  bool play(const glz_play* plays, uint32_t n, int mode, Error& err);
  // A normal set (Deformers::pack_normals, install_normals): the rule runs once, and the scene then does what update_vertices(REFIT) does
  // after its upload over the set's range.  From then on update_vertices, pose_skins and animate run the set's two kernels after their own
  // writes and before the derivatives whenever the span they wrote overlaps the set's reach.  The id, or -1 with the error set.
  int add_normals(const glz_normals& set, Error& err);
  bool read_vertices(uint32_t first, uint32_t n, glz_vertex* out, Error& err);   // as the device holds them
  // The host copy with its vertices current.  `data` itself may be behind the device after pose_skins (never in its counts, transforms,
  // indices, materials or lights); everything that reads the CONTENTS of data.vertices goes through here, which reads the stale span back
  // (that span, no more) the first time it is asked after a pose.
  const SceneData* host_data(Error& err);
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
  // before sources() goes to a call of accel_ that may read the mirror's vertices: a two-level scene's instance boxes come from them
  bool mirror_for_accel(Error& err) { return !accel_.two_level() || host_data(err) != nullptr; }

  Deformers::Sources deformer_sources() const { return Deformers::Sources{instance->device, instance->stream, geometry_.vertices.ptr, data}; }
  // What update_vertices, run_animation, play and add_normals share.  The beginning: the mode's check, the device, the mirror where
  // `mirror_first` says so, compose() on every way out, the refit's preparation and the timer.  Then `write(stream)`, the caller's own
  // step, which puts new vertices on the device.  The tail: the normal sets the written span [first, first + count) reaches (or the set
  // `only` alone, if it is not negative by then), the derivatives, the mirror where it did not come first, and the structure's update over the span as the sets widened it.
  template <class Write>
  bool update_geometry(const char* who, int mode, bool mirror_first, const int& only, uint32_t first, uint32_t count, Write&& write, Error& err);
  bool run_animation(const glz_animation& anim, int mode, const char* who, Error& err);   // pose_skins and animate
  void mark_stale(uint32_t first, uint32_t count);   // joins a span with the one of data.vertices that is already behind the device
  uint32_t stale_first_ = 0, stale_count_ = 0;   // the span of data.vertices that is behind the device (count 0: none)

  Geometry geometry_;
  Textures textures_;
  ShadingTables tables_;
  Accel accel_;
  Deformers deformers_;
};

}  // namespace glz
