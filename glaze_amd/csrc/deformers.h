// The vertex deformers of a scene: skins, morph targets, normal sets, and the skeletons and clips that make a skin's bones on the device
// (skin.h, morph.h, normals.h and clip.h hold the rules and the layouts, kernels_deform.hip, kernels_normals.hip and kernels_clip.hip
// the kernels).  It owns their device buffers, the host copies that replicas on other devices
// are made from, their ids and what a call uploads; what they deform -- the scene's vertex buffer -- belongs to the scene and comes in
// as a Sources with every call that touches it.  The structure's follow-up and the host mirror are the scene's.
#pragma once
#include <map>
#include <vector>

#include "clip.h"
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
  // ---- skeletons and clips: a skin's bone table, and its morph's weight table, made on the device from keyframes (clip.h) ----
  // A skeleton on a skin: parents, inverse bind matrices and root are checked and uploaded once with the level table made of them, and
  // the world and bone tables are allocated (the bone table for the larger blend mode).  A clip on a skeleton: its keys, uploaded once.
  // Each returns its id (>= 0, counting up, never reused), or -1 with the error set; GLZ_E_ARG (nothing changes): see
  // glz_renderer_add_skeleton.  remove_skeleton frees the skeleton's clips with it.
  int add_skeleton(const Sources& s, const glz_skeleton& skeleton, Error& err);
  bool remove_skeleton(int id, Error& err);
  int add_clip(const Sources& s, const glz_clip& clip, Error& err);
  bool remove_clip(int id, Error& err);
  // The checks of a play list (glz_renderer_play lists them: null, none, unknown clip, two clips of one skeleton, a non-finite time) and
  // the span [first, first + count) it writes
  bool played_span(const glz_play* plays, uint32_t n, const char* who, uint32_t& first, uint32_t& count, Error& err) const;
  // What a play list's kernels need uploaded per call: the table of (clip, k0, k1, u, blend), alive until the stream has run them
  struct PlayUploads {
    std::vector<ClipPlay> records;   // the host array the table is copied from (first, so released last)
    DeviceBuffer<ClipPlay> table;
  };
  // Every kernel of one (checked) play list into `span`, which holds the vertices from span_first on: k_clip_bones once for all the
  // plays, then each clip's skin by the kernel animate_into would use, its bone and weight pointers aimed at the tables k_clip_bones wrote.
  bool play_into(const glz_play* plays, uint32_t n, float4* span, uint32_t span_first, PlayUploads& up, hipStream_t st, Error& err) const;
  bool play(const Sources& s, const glz_play* plays, uint32_t n, Error& err) { return play_into(plays, n, s.vertices, 0, play_uploads_, s.stream, err); }
  // k_clip_bones alone for one (checked) play: the bone table as the device holds it afterwards, post::bone_rows(blend) float4 a bone,
  // and the weight table of a clip with a weight track (weights_out may be null).  (glz_debug_clip_bones)
  bool clip_bones(const Sources& s, const glz_play& play, float* rows_out, float* weights_out, Error& err) const;
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
  // everything that makes `src`'s skins, then its morphs, its normal sets, its skeletons and its clips, here (a replica on another device, made of src's current
  // vertices): same ids, same bind poses and bases, same blend modes
  bool copy_from(const Sources& s, const Deformers& src, Error& err);
  // ---- timing hooks: device-event time of `reps` launches after one that is not timed, divided by reps; the scene is untouched ----
  // k_skin (k_skin_dq) of one (checked) pose alone, into a scratch buffer (glz_debug_skin_timing)
  bool time_skin(const Sources& s, const glz_pose& pose, uint32_t reps, float* kernel_ms, Error& err) const;
  // k_clip_bones alone, one launch for the (checked) plays; their table goes up before the timed span (glz_debug_clip_timing)
  bool time_clip(const Sources& s, const glz_play* plays, uint32_t n, uint32_t reps, float* kernel_ms, Error& err) const;
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
    int skeleton = -1;             // the skeleton's id
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
  struct SkeletonHost {
    int skin = -1;
    uint32_t n_bones = 0;
    std::vector<int32_t> parents;
    std::vector<float4> inverse_bind;               // three rows a bone (post::affine_of), then root's three rows
    std::vector<uint32_t> level_bones, level_offsets;   // post::clip_levels
  };
  struct Skeleton {
    SkeletonHost h;
    DeviceBuffer<int32_t> parents;
    DeviceBuffer<uint32_t> level_bones, level_offsets;
    DeviceBuffer<float4> inverse_bind, world, bones;   // world: three rows a bone; bones: the skin's table, sized for either blend mode
  };
  struct ClipHost {
    int skeleton = -1;
    uint32_t n_keys = 0, n_targets = 0;
    std::vector<float> times, translations, rotations, scales, morph_weights;   // scales, morph_weights: empty where the clip has none
  };
  struct Clip {
    ClipHost h;
    DeviceBuffer<float> translations, rotations, scales, morph_weights, weights;   // weights: the table k_clip_bones writes, n_targets
    DeviceBuffer<ClipArgs> args;   // one: what k_clip_bones reads of this clip and its skeleton
  };
  // the device half of add_* and copy_from: every buffer of the record, or none of it.  replica: the vertices it owns come from the host
  // copy; else from the scene's vertex buffer, and the host copy is read from there
  int install_skin(const Sources& s, int id, SkinHost&& h, bool replica, Error& err);
  int install_morph(const Sources& s, int id, MorphHost&& h, bool replica, Error& err);
  int install_normals(const Sources& s, int id, post::NormalLayout&& layout, Error& err);
  int install_skeleton(const Sources& s, int id, SkeletonHost&& h, Error& err);
  int install_clip(const Sources& s, int id, ClipHost&& h, Error& err);
  // One launch of k_deform: the morph under `weights` (null: no morph step), then the (checked) pose of its skin (null: no skin step),
  // whose bones go up packed for the skin's blend mode through `bones`; into `span`, which holds the vertices from span_first on.
  // `packed` and `bones` (null with no pose) must live until the stream has run the kernel.
  bool deform(const Morph* morph, const float* weights, const glz_pose* pose, std::vector<float4>* packed, DeviceBuffer<float4>* bones, float4* span,
              uint32_t span_first, hipStream_t st, Error& err) const;
  // The launch itself, from tables that are on the device already: `weights` of the morph (null: no morph step), `bones` of the skin
  // (null: no skin step) in its blend mode's layout.  deform's second half, and all of a played skin's.
  bool deform_tables(const Morph* morph, const float* weights, const Skin* skin, const float4* bones, float4* span, uint32_t span_first, hipStream_t st, Error& err) const;
  // the play list's table into `up`, on its way up: each clip's key choice for its time, and its skin's blend mode now
  bool upload_plays(const glz_play* plays, uint32_t n, PlayUploads& up, hipStream_t st, Error& err) const;
  static NormalArgs normal_args(const NormalSet& s) { return NormalArgs{s.faces.ptr, s.layout.n_faces, s.counts.ptr, s.slices.ptr, s.rows.ptr, s.layout.n_vertices}; }

  std::map<int, Skin> skins_;
  std::map<int, Morph> morphs_;
  std::map<int, NormalSet> normals_;
  std::map<int, Skeleton> skeletons_;
  std::map<int, Clip> clips_;
  int next_skin_ = 0, next_morph_ = 0, next_normals_ = 0, next_skeleton_ = 0, next_clip_ = 0;
  AnimationUploads uploads_;   // what the scene's own animate / pose_skins calls send up
  PlayUploads play_uploads_;   // what the scene's own play calls send up
};

}  // namespace glz
