// The vertex deformers of a scene: skins, morph targets and normal sets (skin.h, morph.h and normals.h hold the rules and the layouts,
// kernels_deform.hip and kernels_normals.hip the kernels).  It owns their device buffers, the host copies that replicas on other devices
// are made from, their ids and what a call uploads; what they deform -- the scene's vertex buffer -- belongs to the scene and comes in
// as a Sources with every call that touches it.  The structure's follow-up and the host mirror are the scene's.
#pragma once
#include <map>
#include <vector>

#include "hip_util.h"
#include "kernels.h"
#include "morph.h"
#include "normals.h"
#include "parser.h"

namespace glz {

class Deformers {
 public:
  struct Sources {
    int device;
    hipStream_t stream;
    float4* vertices;        // the scene's vertex buffer, two float4 a vertex
    const SceneData& data;   // the vertex count; indices and meshes for post::pack_normals
  };
  // ---- skinned meshes ----
  // A skin over the vertices [first_vertex, first_vertex + n_vertices): its bind pose is what the DEVICE holds there now (copied device to
  // device into a buffer the skin owns), joints and weights are uploaded once.  Returns the skin's id (>= 0), or -1 with the error set;
  // GLZ_E_ARG (nothing changes): see glz_renderer_add_skin.  Ids count up and are never reused, so the replicas of a scene, told the same
  // calls in the same order, give the same ids.
  int add_skin(const Sources& s, const glz_skin& skin, Error& err);
  bool remove_skin(int id, Error& err);   // the vertices stay as they are
  // A skin's blend mode (GLZ_SKIN_*; a new skin is GLZ_SKIN_LINEAR).  Setting it writes no vertex: no bones are kept between calls, so the
  // next pose, animation or previous-pose pass packs its bones for the mode and runs the mode's kernel.  GLZ_E_ARG (nothing changes): no
  // such skin, an unknown mode; skin_blend returns -1 then.
  bool set_skin_blend(int id, int blend, Error& err);
  int skin_blend(int id, Error& err) const;
  // ---- morph targets ----
  // A morph over [first_vertex, first_vertex + n_vertices): the targets are checked and transposed into the layout (post::pack_morph) and
  // uploaded once.  Free-standing (skin == -1): its base is what the DEVICE holds in the range now, copied into a buffer the morph owns;
  // attached: its base is the skin's bind buffer.  Returns the id (>= 0, counting up, never reused), or -1 with the error set; GLZ_E_ARG
  // (nothing changes): see glz_renderer_add_morph.
  int add_morph(const Sources& s, const glz_morph& morph, Error& err);
  bool remove_morph(int id, Error& err);   // the vertices stay as they are
  // ---- animations: morph weights and poses in one call; a pose list is an animation with no morph named ----
  // The checks of an animation (glz_renderer_animate lists them: null, none, unknown id, an id twice, another bone or target count, an
  // attached morph without its skin's pose) and the span [first, first + count) it writes
  bool animated_span(const glz_animation* anim, const char* who, uint32_t& first, uint32_t& count, Error& err) const;
  // What an animation's kernels need uploaded per call: owned by whoever runs them, alive until the stream has run them
  struct AnimationUploads {
    std::vector<std::vector<float4>> packed;   // the host arrays the bone tables are copied from (first, so released last)
    std::vector<DeviceBuffer<float4>> bones;   // one table per pose
    std::vector<DeviceBuffer<float>> weights;  // one table per named morph
  };
  // Every kernel of one (checked) animation into `span`, which holds the vertices from span_first on: each named free-standing morph by
  // k_morph from its base, each named skin by k_skin (k_skin_dq in that mode) from its bind pose, or by k_morph_skin (k_morph_skin_dq)
  // where its morph is named too.  The span is the scene's vertex buffer (animate), or motion_pass's previous-vertex buffer.
  bool animate_into(const glz_animation& anim, float4* span, uint32_t span_first, AnimationUploads& up, hipStream_t st, Error& err) const;
  // (the uploads are the part's own, reused while the calls name as much; they outlive the copies when the caller waits for the stream)
  bool animate(const Sources& s, const glz_animation& anim, Error& err) { return animate_into(anim, s.vertices, 0, uploads_, s.stream, err); }
  // ---- vertex normals from deformed positions ----
  // A normal set over [first_vertex, first_vertex + n_vertices), in two steps so that the scene can prepare the structure's update between
  // them: the checks (GLZ_E_ARG, see glz_renderer_add_normals) with the face list and the rows (post::pack_normals), then the upload, which
  // returns the id (>= 0, counting up, never reused) or -1 with the error set.  No kernel runs here: run_normals(only = id) is the
  // caller's, and from then on every write whose span overlaps the set's reach (the lowest to the highest corner of its faces) is
  // followed by run_normals.
  bool pack_normals(const Sources& s, const glz_normals& set, post::NormalLayout& layout, Error& err) const;
  int install_normals(const Sources& s, post::NormalLayout&& layout, Error& err);
  bool remove_normals(int id, Error& err);   // the vertices stay as they are
  // The two kernels of every set whose reach overlaps the written span [first, first + count) -- or of the set `only` alone, if not
  // negative -- on the stream; first / count come back as the union of the span and those sets' ranges: what the structure's update and
  // the host mirror have to know as changed.  ran: whether any set's normals were written.
  bool run_normals(const Sources& s, int only, uint32_t& first, uint32_t& count, bool& ran, Error& err) const;
  // everything that makes `src`'s skins, then its morphs, then its normal sets, here (a replica on another device, made of src's current
  // vertices): same ids, same bind poses and bases, same blend modes
  bool copy_from(const Sources& s, const Deformers& src, Error& err);
  // ---- timing hooks: device-event time of `reps` launches after one that is not timed, divided by reps; the scene is untouched ----
  // k_skin (k_skin_dq) of one (checked) pose alone, into a scratch buffer (glz_debug_skin_timing)
  bool time_skin(const Sources& s, const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const;
  // One of the morph kernels alone, into a scratch buffer (glz_debug_morph_timing); *bytes: what one launch moves, by the layout's own count
  bool time_morph(const Sources& s, const glz_animation& one, uint32_t reps, float* kernel_ms, uint64_t* bytes, Error& err) const;
  // Each of the two kernels of one set alone: k_face_vectors into a scratch buffer of face vectors, k_vertex_normals from it into a
  // scratch copy of the set's vertices.  ms / bytes: [0] the face kernel, [1] the vertex kernel; bytes by the layout's own count
  // (glz_debug_normals_timing)
  bool time_normals(const Sources& s, int id, uint32_t reps, float ms[2], uint64_t bytes[2], Error& err) const;

 private:
  // Each record: what a replica on another device, created later (DeviceGroup), is made from -- and the device buffers
  struct SkinHost {
    uint32_t first = 0, n = 0, n_bones = 0;
    int blend = GLZ_SKIN_LINEAR;   // GLZ_SKIN_*: which rule, bone table and kernel a pose of it uses
    int morph = -1;                // the attached morph's id
    std::vector<glz_vertex> bind;
    std::vector<uint16_t> joints;
    std::vector<float> weights;
  };
  struct Skin {
    SkinHost h;
    DeviceBuffer<float4> bind, weights;   // 2 a vertex; 1 a vertex
    DeviceBuffer<uint2> joints;           // four uint16 a vertex
  };
  struct MorphHost {
    uint32_t first = 0;
    int skin = -1;                 // -1: free-standing, base is its own; else the skin whose bind buffer is the base
    std::vector<glz_vertex> base;  // free-standing only
    post::MorphLayout layout;
  };
  struct Morph {
    MorphHost h;
    DeviceBuffer<float4> base, entries;   // 2 a vertex (free-standing only); the layout's
    DeviceBuffer<uint32_t> counts;
    DeviceBuffer<uint2> slices;
  };
  struct NormalSet {
    post::NormalLayout layout;
    DeviceBuffer<uint32_t> faces, counts, rows;
    DeviceBuffer<uint2> slices;
    DeviceBuffer<float4> face_vectors;   // one a face: k_face_vectors writes it, k_vertex_normals reads it
  };
  // the device half of add_* and copy_from: every buffer of the record, or none of it.  replica: the vertices it owns come from the host
  // copy; else from the scene's vertex buffer, and the host copy is read from there
  int install_skin(const Sources& s, int id, SkinHost&& h, bool replica, Error& err);
  int install_morph(const Sources& s, int id, MorphHost&& h, bool replica, Error& err);
  int install_normals(const Sources& s, int id, post::NormalLayout&& layout, Error& err);
  // One launch of k_deform: the morph under `weights` (null: no morph step), then the (checked) pose of its skin (null: no skin step),
  // whose bones go up packed for the skin's blend mode through `bones`; into `span`, which holds the vertices from span_first on.
  // `packed` and `bones` (null with no pose) must live until the stream has run the kernel.
  bool deform(const Morph* morph, const float* weights, const glz_pose* pose, std::vector<float4>* packed, DeviceBuffer<float4>* bones, float4* span,
              uint32_t span_first, hipStream_t st, Error& err) const;
  static NormalArgs normal_args(const NormalSet& s) { return NormalArgs{s.faces.ptr, s.layout.n_faces, s.counts.ptr, s.slices.ptr, s.rows.ptr, s.layout.n_vertices}; }

  std::map<int, Skin> skins_;
  std::map<int, Morph> morphs_;
  std::map<int, NormalSet> normals_;
  int next_skin_ = 0, next_morph_ = 0, next_normals_ = 0;
  AnimationUploads uploads_;   // what the scene's own animate / pose_skins calls send up
};

}  // namespace glz
