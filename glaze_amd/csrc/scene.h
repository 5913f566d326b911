// RayTraceInstance / RayTraceScene equivalents: device selection, scene upload, and the parts a scene is made of -- the textures
// (textures.h), the shading tables (shading_tables.h) and the acceleration structure (accel.h).
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "accel.h"
#include "device/types.h"
#include "glaze_abi.h"
#include "hip_util.h"
#include "instance_boxes.h"
#include "kernels.h"
#include "morph.h"
#include "normals.h"
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
  // ---- skinned meshes (skin.h holds the rule, kernels_skin.hip the kernel) ----
  // A skin over the vertices [first_vertex, first_vertex + n_vertices): its bind pose is what the DEVICE holds there now (copied device to
  // device into a buffer the skin owns), joints and weights are uploaded once.  Returns the skin's id (>= 0), or -1 with the error set;
  // GLZ_E_ARG (nothing changes): see glz_renderer_add_skin.  Skins are the scene's, as the vertices are; ids count up and are never reused,
  // so the replicas of a scene, told the same calls in the same order, give the same ids.
  int add_skin(const glz_skin& skin, Error& err);
  bool remove_skin(int id, Error& err);   // the vertices stay as they are
  // A skin's blend mode (GLZ_SKIN_*; a new skin is GLZ_SKIN_LINEAR).  Setting it writes no vertex: no bones are kept between calls, so the
  // next pose, animation or previous-pose pass packs its bones for the mode and runs the mode's kernel.  GLZ_E_ARG (nothing changes): no
  // such skin, an unknown mode; skin_blend returns -1 then.
  bool set_skin_blend(int id, int blend, Error& err);
  int skin_blend(int id, Error& err) const;
  // Poses skins (each named once, with the bone count it was added with) and updates the structure once: bones up, k_skin per skin from its
  // bind pose into the vertex buffer, then what update_vertices does after its upload, over the span from the lowest to the highest posed
  // vertex.  The host mirror (data.vertices) is NOT written: the span is marked stale and read back when a reader asks (host_data()).
  bool pose_skins(const glz_pose* poses, uint32_t n_poses, int mode, Error& err);
  // The checks of a set of poses (null, none, unknown id, an id twice, another bone count) and the span [first, first + count) they cover
  bool posed_span(const glz_pose* poses, uint32_t n_poses, const char* who, uint32_t& first, uint32_t& count, Error& err) const;
  // What motion_pass fills its previous-vertex buffer with: k_skin (k_skin_dq for a skin in that mode) of one (checked) pose into `span`, which holds the vertices from
  // span_first on; the packed bones go up through `bones`, which must live until the stream has run the kernel, as must `packed`.
  bool skin_into(const glz_pose& pose, float4* span, uint32_t span_first, std::vector<float4>& packed, DeviceBuffer<float4>& bones, hipStream_t st, Error& err) const;
  bool read_vertices(uint32_t first, uint32_t n, glz_vertex* out, Error& err);   // as the device holds them
  // k_skin of one (checked) pose alone, into a scratch buffer (the scene is untouched): device-event time of `reps` launches after one
  // that is not timed, divided by reps (glz_debug_skin_timing)
  bool time_skin(const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const;
  // The host copy with its vertices current.  `data` itself may be behind the device after pose_skins (never in its counts, transforms,
  // indices, materials or lights); everything that reads the CONTENTS of data.vertices goes through here, which reads the stale span back
  // (that span, no more) the first time it is asked after a pose.
  const SceneData* host_data(Error& err);
  // everything that makes `src`'s skins, on this scene (a replica on another device): same ids, same bind poses, same blend modes
  bool copy_skins(const Scene& src, Error& err);
  // ---- morph targets (morph.h holds the rule and the layout, kernels_morph.hip the kernels) ----
  // A morph over [first_vertex, first_vertex + n_vertices): the targets are checked and transposed into the layout (post::pack_morph) and
  // uploaded once.  Free-standing (skin == -1): its base is what the DEVICE holds in the range now, copied into a buffer the morph owns;
  // attached: its base is the skin's bind buffer.  Returns the id (>= 0, counting up, never reused), or -1 with the error set; GLZ_E_ARG
  // (nothing changes): see glz_renderer_add_morph.
  int add_morph(const glz_morph& morph, Error& err);
  bool remove_morph(int id, Error& err);   // the vertices stay as they are
  // Morphs and poses in one update of the structure (glz_renderer_animate): each named free-standing morph by k_morph from its base, each
  // named skin by k_skin, or by k_morph_skin where its morph is named too, into the vertex buffer; then what pose_skins does after its
  // kernels, over the span from the lowest to the highest vertex written.  pose_skins is this with no morph named.
  bool animate(const glz_animation& anim, int mode, Error& err);
  // The checks of an animation (glz_renderer_animate lists them; the poses' are posed_span's) and the span it writes
  bool animated_span(const glz_animation* anim, const char* who, uint32_t& first, uint32_t& count, Error& err) const;
  // What an animation's kernels need uploaded per call: owned by whoever runs them, alive until the stream has run them
  struct AnimationUploads {
    std::vector<std::vector<float4>> packed;   // the host arrays the bone tables are copied from (first, so released last)
    std::vector<DeviceBuffer<float4>> bones;   // one table per pose
    std::vector<DeviceBuffer<float>> weights;  // one table per named morph
  };
  // Every kernel of one (checked) animation into `span`, which holds the vertices from span_first on: the scene's vertex buffer
  // (animate), or motion_pass's previous-vertex buffer
  bool animate_into(const glz_animation& anim, float4* span, uint32_t span_first, AnimationUploads& up, hipStream_t st, Error& err) const;
  // One of the morph kernels alone, into a scratch buffer (glz_debug_morph_timing): timed as time_skin times k_skin; *bytes: what one
  // launch moves, by the layout's own count
  bool time_morph(const glz_animation& one, uint32_t reps, float* kernel_ms, uint64_t* bytes, Error& err) const;
  // everything that makes `src`'s morphs, on this scene (a replica on another device), after copy_skins: same ids, same bases
  bool copy_morphs(const Scene& src, Error& err);
  // ---- vertex normals from deformed positions (normals.h holds the rule and the layout, kernels_normals.hip the kernels) ----
  // A normal set over [first_vertex, first_vertex + n_vertices): the face list and the rows are made once (post::pack_normals) and
  // uploaded; the rule runs once, and the scene then does what update_vertices(REFIT) does after its upload over the set's range.  From
  // then on update_vertices, pose_skins and animate run the set's two kernels after their own writes and before the derivatives whenever
  // the span they wrote overlaps the set's reach (the lowest to the highest corner of its faces).  Returns the id (>= 0, counting up,
  // never reused), or -1 with the error set; GLZ_E_ARG (nothing changes): see glz_renderer_add_normals.
  int add_normals(const glz_normals& set, Error& err);
  bool remove_normals(int id, Error& err);   // the vertices stay as they are
  // Each of the two kernels of one set alone, `reps` times after one launch that is not timed: k_face_vectors into a scratch buffer of
  // face vectors, k_vertex_normals from it into a scratch copy of the set's vertices (the scene is untouched).  ms / bytes: [0] the
  // face kernel, [1] the vertex kernel; bytes by the layout's own count (glz_debug_normals_timing)
  bool time_normals(int id, uint32_t reps, float ms[2], uint64_t bytes[2], Error& err) const;
  // everything that makes `src`'s normal sets, on this scene (a replica on another device, made of src's current vertices): same ids
  bool copy_normals(const Scene& src, Error& err);
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

  struct Skin {
    uint32_t first = 0, n = 0, n_bones = 0;
    int blend = GLZ_SKIN_LINEAR;                 // GLZ_SKIN_*: which rule, bone table and kernel a pose of it uses
    DeviceBuffer<float4> bind, weights;          // 2 a vertex; 1 a vertex
    DeviceBuffer<uint2> joints;                  // four uint16 a vertex
    // host copies, for the replicas on other devices that are created later (DeviceGroup)
    std::vector<glz_vertex> h_bind;
    std::vector<uint16_t> h_joints;
    std::vector<float> h_weights;
    int morph = -1;   // the attached morph's id
  };
  struct Morph {
    uint32_t first = 0, n = 0, n_targets = 0;
    int skin = -1;                         // -1: free-standing, base is its own; else the skin whose bind buffer is the base
    uint64_t n_entries = 0;
    DeviceBuffer<float4> base, entries;    // 2 a vertex (free-standing only); the layout's
    DeviceBuffer<uint32_t> counts;
    DeviceBuffer<uint2> slices;
    // host copies, for the replicas on other devices that are created later (DeviceGroup)
    std::vector<glz_vertex> h_base;
    post::MorphLayout layout;
  };
  int install_morph(int id, uint32_t first, int skin, std::vector<glz_vertex>&& base, post::MorphLayout&& layout, const float4* device_base, Error& err);
  MorphArgs morph_args(const Morph& m, const float* weights) const;
  // the bones of a (checked) pose, packed for its skin's blend mode and on their way up through `bones` (post::bone_rows float4 a bone)
  bool upload_bones(const glz_pose& pose, std::vector<float4>& packed, DeviceBuffer<float4>& bones, hipStream_t st, Error& err) const;
  bool run_animation(const glz_animation& anim, int mode, const char* who, Error& err);   // pose_skins and animate
  AnimationUploads uploads_;   // what the scene's own animate / pose_skins calls send up
  std::map<int, Morph> morphs_;
  int next_morph_ = 0;
  struct NormalSet {
    post::NormalLayout layout;               // (kept whole on the host for the replicas on other devices that are created later)
    DeviceBuffer<uint32_t> faces, counts, rows;
    DeviceBuffer<uint2> slices;
    DeviceBuffer<float4> face_vectors;       // one a face: k_face_vectors writes it, k_vertex_normals reads it
  };
  int install_normals(int id, post::NormalLayout&& layout, Error& err);
  static NormalArgs normal_args(const NormalSet& s);
  // The two kernels of every set whose reach overlaps the written span [first, first + count), on `st`; first / count come back as the
  // union of the span and those sets' ranges: what the structure's update and the host mirror have to know as changed
  bool run_normals(uint32_t& first, uint32_t& count, hipStream_t st, Error& err);
  void mark_stale(uint32_t first, uint32_t count);   // joins a span with the one of data.vertices that is already behind the device
  std::map<int, NormalSet> normals_;
  int next_normals_ = 0;
  int install_skin(int id, uint32_t first, std::vector<glz_vertex>&& bind, std::vector<uint16_t>&& joints, std::vector<float>&& weights, uint32_t n_bones,
                   int blend, const float4* device_bind, Error& err);
  std::map<int, Skin> skins_;
  int next_skin_ = 0;
  uint32_t stale_first_ = 0, stale_count_ = 0;   // the span of data.vertices that is behind the device (count 0: none)

  Geometry geometry_;
  Textures textures_;
  ShadingTables tables_;
  Accel accel_;
};

}  // namespace glz
