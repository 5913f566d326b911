// The post stage of a renderer (kernels_post.hip): the first-hit pass with its feature buffers, the guide chain, the a-trous filter, the
// firefly rejection, motion and reprojection.  It runs on the renderer's own device only, over the FULL frame whatever the partition, on
// the instance's stream.  Its buffers and settings are its own; device, stream, scene, frame size and camera are the renderer's, read on
// every call -- a new scene, camera or set of transforms needs no word to the stage, a new resolution only release().
#pragma once
#include "hip_util.h"
#include "kernels.h"
#include "scene.h"

namespace glz {

class Renderer;

// Previous vertices made on the device (glz_renderer_read_motion_posed / reproject_posed, *_animated): the skins as the PREVIOUS bones pose them.  The
// buffer k_motion_deform reads then holds the span from the lowest to the highest posed vertex: the scene's current vertices copied
// device to device (so a gap between skins holds current values), then k_skin of every named skin with these bones.
struct PrevPoses {
  const glz_pose* poses = nullptr;
  uint32_t n = 0;
  bool given = false;   // a *_posed / *_animated call: the state must bring no vertices, and the poses are checked as pose_skins checks them
  // *_animated: the previous morph weights as well, and the whole checked and run as glz_renderer_animate does (Scene::animate_into)
  const glz_morph_weights* morphs = nullptr;
  uint32_t n_morphs = 0;
  glz_animation animation() const { return glz_animation{morphs, n_morphs, poses, n}; }
};

class PostStage {
 public:
  explicit PostStage(const Renderer& r) : r_(r) {}
  void release();   // every buffer; each comes back on first use

  // ---- first-hit feature buffers and the denoiser ----
  bool read_aov(int which, float* out, Error& err);                   // runs the first-hit pass; GLZ_AOV_*
  bool set_denoise(const glz_denoise_params* p, Error& err);          // null = defaults; accumulation goes on
  const glz_denoise_params& denoise() const { return denoise_; }
  // firefly rejection (glz_despeckle_params): enabled = ahead of the filter in read_denoised; null = defaults; accumulation goes on
  bool set_despeckle(bool enabled, const glz_despeckle_params* p, Error& err);
  int despeckle(glz_despeckle_params* out) const;                      // the enabled flag
  // The first-hit pass, then on `frame` (device; the renderer's gathered result) the a-trous passes, with the rejection ahead of them when
  // it is enabled (filter), or demodulation + rejection with no filter pass (!filter).  Returns the device frame that holds the outcome
  // once the stream has drained, null on failure.  marks: null, or GLZ_POST_TIMING_SLOTS + 2 events -- three around the first-hit pass's
  // kernels, 2 + iterations around the filter's; such a timed run never includes the rejection.
  const float4* filtered(const float4* frame, bool filter, hipEvent_t* marks, Error& err);
  // motion vectors and history reprojection (glz_reproject_params; reproject.h): the first-hit trace and k_motion against the caller's
  // previous state -- camera, transforms (null = the scene's own) and vertices (null = the meshes did not deform; else k_motion_deform on the
  // uploaded array) -- then, for reproject, k_reproject on the three uploaded previous frames
  bool read_motion(const glz_previous_state& prev, float* out, Error& err, const PrevPoses& posed = {});
  bool time_motion(const glz_previous_state& prev, float* kernel_ms, Error& err);   // k_motion / k_motion_deform alone, device events
  bool reproject(const glz_previous_state& prev, const float* prev_color, const float* prev_aov0, const float* prev_aov1, const glz_reproject_params* params, float* out,
                 Error& err, const PrevPoses& posed = {});
  bool camera_rays(float off_x, float off_y, float* origins3, float* dirs3, Error& err);   // camera_ray() of every pixel, on the device
  // which surface the feature buffers describe (GLZ_GUIDE_*, glaze_abi.h holds the specification); accumulation goes on
  bool set_guide_mode(int mode, uint32_t max_bounces, Error& err);
  int guide_mode(uint32_t* max_bounces_out) const;
  // the rays of one segment of every pixel's guide chain under the mode and cap in force (glz_debug_guide_chain)
  bool guide_chain(uint32_t segment, float* origins3, float* dirs3, uint8_t* alive, Error& err);

 private:
  // what the first-hit pass launches k_motion with, between the trace and whatever reuses the hit buffers
  struct MotionStep {
    post::ProjectConstants prev;
    const float4* prev_o2w;   // device, or null = the scene's own
    const float4* prev_vertices;            // device, or null = the meshes did not deform: the previous contents of the scene's vertices
    uint32_t first_vertex, n_vertices;      //   [first_vertex, first_vertex + n_vertices), two float4 each
    float4* out;              // device
    hipEvent_t* marks;        // null, or two events recorded around k_motion
  };
  struct FirstHitRequest {
    hipEvent_t* marks = nullptr;                      // null, or 3 events around the trace and what follows it
    uint32_t last_list = GLZ_GUIDE_MAX_BOUNCES + 1;   // launch_guide_chain's: the chain stops once this list is written
    const MotionStep* motion = nullptr;               // null, or motion_pass()'s k_motion
  };
  // The first-hit pass over the FULL frame on this device, whatever the partition: centre rays, closest hits, attributes -> aov0_ / aov1_.
  // Recomputed on every request, never cached; its buffers are private (allocated on first use, released by release()).
  // In GLZ_GUIDE_THROUGH_SPECULAR the chain's kernels take the attribute kernel's place (launch_guide_chain).
  bool first_hit_pass(const FirstHitRequest& req, Error& err);
  void post_args(LaunchArgs& a) const;
  // what a motion pass uploads of the caller's previous state: owned by the call and released with it
  struct PrevBuffers {
    Deformers::AnimationUploads animation;           // the bone and weight tables of the previous poses and morphs (its host arrays first, so released last)
    DeviceBuffer<float4> o2w, vertices;
  };
  bool motion_pass(const glz_previous_state& prev, PrevBuffers& uploaded, DeviceBuffer<float4>& motion, Error& err, hipEvent_t* marks = nullptr,
                   const PrevPoses& posed = {});
  GuideLists guide_lists() const { return GuideLists{{guide_o_[0].ptr, guide_o_[1].ptr}, {guide_d_[0].ptr, guide_d_[1].ptr}, guide_count_.ptr}; }

  const Renderer& r_;
  DeviceBuffer<float4> fh_hit_, aov0_, aov1_, dn_ping_, dn_pong_, dn_out_;
  DeviceBuffer<uint32_t> fh_inst_, fh_overflow_;
  glz_denoise_params denoise_ = post::denoise_defaults();
  glz_despeckle_params despeckle_ = post::despeckle_defaults();
  bool despeckle_on_ = false;
  int guide_mode_ = GLZ_GUIDE_FIRST_HIT;
  uint32_t guide_bounces_ = 4;
  DeviceBuffer<float4> guide_o_[2], guide_d_[2];   // the chain's ray lists (GuideLists), allocated on first use in GLZ_GUIDE_THROUGH_SPECULAR
  DeviceBuffer<uint32_t> guide_count_;
  uint32_t guide_blocks_ = 0;                      // the chain's grid in the last pass
};

}  // namespace glz
