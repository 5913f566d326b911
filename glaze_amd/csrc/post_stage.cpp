// The post stage of a renderer -- see post_stage.h.
#include "post_stage.h"

#include <cstring>

#include "denoise.h"
#include "renderer.h"

namespace glz {

namespace {
// A group of buffers of n entries each is there at that size, or is allocated now.  All or nothing: a failure releases the group, so the
// next request starts over instead of meeting a buffer that is not there.
template <class... Buffers>
bool present(size_t n, const char* what, Error& err, Buffers&... buffers) {
  if (((buffers.ptr != nullptr && buffers.count == n) && ...)) return true;
  if (hip_ok(alloc_each(n, buffers...), what, err)) return true;
  (buffers.release(), ...);
  return false;
}
bool bad_argument(Error& err, const char* message) {
  return err.fail(GLZ_E_ARG, message);
}
}  // namespace

void PostStage::release() {
  fh_hit_.release(); fh_inst_.release(); fh_overflow_.release();
  aov0_.release(); aov1_.release();
  dn_ping_.release(); dn_pong_.release(); dn_out_.release();
  for (int i = 0; i < 2; ++i) { guide_o_[i].release(); guide_d_[i].release(); }
  guide_count_.release();
}

// what the post kernels read of LaunchArgs: the scene, the camera, the frame's size and projection, a FULL-frame tile map
void PostStage::post_args(LaunchArgs& a) const {
  memset(&a, 0, sizeof(a));
  a.scene = r_.scene()->dev;
  a.cam = r_.camera_consts();
  a.frame.scene_size[0] = (float)r_.width();
  a.frame.scene_size[1] = (float)r_.height();
  a.frame.camera_persp = r_.perspective() ? 1u : 0u;
  a.map = make_tile_map(r_.width(), r_.height(), 0, 1);
}

bool PostStage::first_hit_pass(const FirstHitRequest& req, Error& err) {
  hipEvent_t* const marks = req.marks;
  if (!hip_ok(hipSetDevice(r_.instance()->device), "hipSetDevice", err)) return false;
  LaunchArgs a;
  post_args(a);
  const size_t n = (size_t)r_.width() * r_.height();
  if (!present(n, "alloc first-hit records", err, fh_hit_, fh_inst_) || !present(n, "alloc feature buffers", err, aov0_, aov1_)) return false;
  const uint32_t blocks = first_hit_grid_blocks(a.map.n_local_pixels);
  const uint32_t od = r_.scene()->accel().stack_overflow_depth;
  const size_t spill = (size_t)blocks * kTraceBlock * od;   // the scene may have changed since the last pass
  if (fh_overflow_.ptr == nullptr || fh_overflow_.count != spill)
    if (!hip_ok(fh_overflow_.alloc(spill), "alloc traversal spill", err)) {
      fh_overflow_.release();
      return false;
    }
  const bool chain = guide_mode_ == GLZ_GUIDE_THROUGH_SPECULAR;
  if (chain && (!present(n, "alloc guide ray lists", err, guide_o_[0], guide_o_[1], guide_d_[0], guide_d_[1]) ||
                !present(kGuideCountWords, "alloc guide ray lists", err, guide_count_)))
    return false;
  a.st.overflow = fh_overflow_.ptr;
  a.st.overflow_depth = od;
  hipStream_t st = r_.instance()->stream;
  // every record starts as a miss: the attribute kernel follows a record's leaf index into the scene's arrays
  if (!hip_ok(hipMemsetAsync(fh_hit_.ptr, 0xFF, sizeof(float4) * n, st), "clear first-hit records", err)) return false;
  if (marks) (void)hipEventRecord(marks[0], st);
  if (!hip_ok(launch_first_hit(st, a, blocks, fh_hit_.ptr, fh_inst_.ptr), "k_first_hit", err)) return false;
  if (marks) (void)hipEventRecord(marks[1], st);
  if (req.motion) {
    const MotionStep& m = *req.motion;
    if (m.marks) (void)hipEventRecord(m.marks[0], st);
    if (!hip_ok(launch_motion(st, a, fh_hit_.ptr, fh_inst_.ptr, m.prev_o2w, m.prev, m.out, m.prev_vertices, m.first_vertex, m.n_vertices), "k_motion", err)) return false;
    if (m.marks) (void)hipEventRecord(m.marks[1], st);
  }
  if (chain) {
    guide_blocks_ = guide_grid_blocks(a.map.n_local_pixels, blocks);
    if (!hip_ok(launch_guide_chain(st, a, guide_blocks_, guide_bounces_, req.last_list, fh_hit_.ptr, fh_inst_.ptr, guide_lists(), aov0_.ptr, aov1_.ptr), "k_guide_continue", err))
      return false;
  } else if (!hip_ok(launch_first_hit_attributes(st, a, fh_hit_.ptr, fh_inst_.ptr, aov0_.ptr, aov1_.ptr), "k_first_hit_attributes", err)) {
    return false;
  }
  if (marks) (void)hipEventRecord(marks[2], st);
  return true;
}

bool PostStage::set_guide_mode(int mode, uint32_t max_bounces, Error& err) {
  if (mode != GLZ_GUIDE_FIRST_HIT && mode != GLZ_GUIDE_THROUGH_SPECULAR) return bad_argument(err, "unknown guide mode (GLZ_GUIDE_FIRST_HIT or GLZ_GUIDE_THROUGH_SPECULAR)");
  if (mode == GLZ_GUIDE_THROUGH_SPECULAR && (max_bounces < 1 || max_bounces > GLZ_GUIDE_MAX_BOUNCES))
    return bad_argument(err, "guide mode: max_bounces must be 1 .. GLZ_GUIDE_MAX_BOUNCES");
  guide_mode_ = mode;
  if (mode == GLZ_GUIDE_THROUGH_SPECULAR) guide_bounces_ = max_bounces;
  return true;
}
int PostStage::guide_mode(uint32_t* max_bounces_out) const {
  if (max_bounces_out) *max_bounces_out = guide_bounces_;
  return guide_mode_;
}

bool PostStage::guide_chain(uint32_t segment, float* origins3, float* dirs3, uint8_t* alive, Error& err) {
  const size_t n = (size_t)r_.width() * r_.height();
  if (segment == 0) {   // the camera rays: every pixel has them
    memset(alive, 1, n);
    return camera_rays(0.5f, 0.5f, origins3, dirs3, err);
  }
  memset(origins3, 0, sizeof(float) * 3 * n);
  memset(dirs3, 0, sizeof(float) * 3 * n);
  memset(alive, 0, n);
  if (guide_mode_ != GLZ_GUIDE_THROUGH_SPECULAR || segment > guide_bounces_ || n == 0) return true;
  if (!first_hit_pass({nullptr, segment}, err)) return false;   // up to the list of this segment
  DeviceBuffer<float> d_o, d_d;
  DeviceBuffer<uint8_t> d_alive;
  if (!hip_ok(d_o.alloc(3 * n), "alloc", err) || !hip_ok(d_d.alloc(3 * n), "alloc", err) || !hip_ok(d_alive.alloc(n), "alloc", err)) return false;
  hipStream_t st = r_.instance()->stream;
  if (!hip_ok(hipMemsetAsync(d_o.ptr, 0, sizeof(float) * 3 * n, st), "guide chain", err) || !hip_ok(hipMemsetAsync(d_d.ptr, 0, sizeof(float) * 3 * n, st), "guide chain", err) ||
      !hip_ok(hipMemsetAsync(d_alive.ptr, 0, n, st), "guide chain", err))
    return false;
  if (!hip_ok(launch_guide_scatter(st, guide_blocks_, guide_lists(), segment, (uint32_t)n, d_o.ptr, d_d.ptr, d_alive.ptr), "k_guide_scatter", err)) return false;
  return r_.to_host({{origins3, d_o.ptr, sizeof(float) * 3 * n}, {dirs3, d_d.ptr, sizeof(float) * 3 * n}, {alive, d_alive.ptr, n}}, "guide chain", err);
}

bool PostStage::read_aov(int which, float* out, Error& err) {
  if (which != GLZ_AOV_NORMAL_DEPTH && which != GLZ_AOV_ALBEDO_INSTANCE) return bad_argument(err, "unknown feature buffer (GLZ_AOV_NORMAL_DEPTH or GLZ_AOV_ALBEDO_INSTANCE)");
  if (!first_hit_pass({}, err)) return false;
  return r_.frame_to_host(which == GLZ_AOV_NORMAL_DEPTH ? aov0_.ptr : aov1_.ptr, out, "read feature buffer", err);
}

bool PostStage::camera_rays(float off_x, float off_y, float* origins3, float* dirs3, Error& err) {
  if (!hip_ok(hipSetDevice(r_.instance()->device), "hipSetDevice", err)) return false;
  LaunchArgs a;
  post_args(a);
  const size_t n = (size_t)r_.width() * r_.height() * 3;
  DeviceBuffer<float> d_o, d_d;
  if (!hip_ok(d_o.alloc(n), "alloc", err) || !hip_ok(d_d.alloc(n), "alloc", err)) return false;
  if (!hip_ok(launch_camera_rays(r_.instance()->stream, a, off_x, off_y, d_o.ptr, d_d.ptr), "k_camera_rays", err)) return false;
  return r_.to_host({{origins3, d_o.ptr, sizeof(float) * n}, {dirs3, d_d.ptr, sizeof(float) * n}}, "camera rays", err);
}

bool PostStage::set_denoise(const glz_denoise_params* p, Error& err) {
  const glz_denoise_params v = p ? *p : post::denoise_defaults();
  if (!post::denoise_params_valid(v)) return bad_argument(err, post::kDenoiseParamsMessage);
  denoise_ = v;
  return true;
}

bool PostStage::set_despeckle(bool enabled, const glz_despeckle_params* p, Error& err) {
  const glz_despeckle_params v = p ? *p : post::despeckle_defaults();
  if (!post::despeckle_params_valid(v)) return bad_argument(err, post::kDespeckleParamsMessage);
  despeckle_ = v;
  despeckle_on_ = enabled;
  return true;
}
int PostStage::despeckle(glz_despeckle_params* out) const {
  if (out) *out = despeckle_;
  return despeckle_on_ ? 1 : 0;
}

const float4* PostStage::filtered(const float4* frame, bool filter, hipEvent_t* marks, Error& err) {
  FirstHitRequest pass;
  pass.marks = marks;
  if (!first_hit_pass(pass, err)) return nullptr;
  const uint32_t w = r_.width(), h = r_.height();
  if (!present((size_t)w * h, "alloc denoiser frames", err, dn_ping_, dn_pong_, dn_out_)) return nullptr;
  hipStream_t st = r_.instance()->stream;
  const hipError_t launched =
      filter ? launch_denoise(st, w, h, denoise_, frame, aov0_.ptr, aov1_.ptr, dn_ping_.ptr, dn_pong_.ptr, dn_out_.ptr, marks ? marks + 3 : nullptr,
                              despeckle_on_ && !marks ? &despeckle_ : nullptr)
             : launch_despeckle(st, w, h, despeckle_, denoise_.eps_albedo, frame, aov0_.ptr, aov1_.ptr, dn_ping_.ptr, dn_out_.ptr);
  return hip_ok(launched, filter ? "k_atrous" : "k_despeckle", err) ? dn_out_.ptr : nullptr;
}

// the checks of read_motion and reproject, the upload of the caller's matrices and vertices, then the first-hit pass with k_motion in it
bool PostStage::motion_pass(const glz_previous_state& prev, PrevBuffers& uploaded, DeviceBuffer<float4>& motion, Error& err, hipEvent_t* marks, const PrevPoses& posed) {
  const glz_camera* prev_camera = prev.camera;
  const glz_transform* prev_transforms = prev.transforms;
  const uint32_t n_prev = prev.n_transforms;
  if (!prev_camera) return bad_argument(err, "motion: the previous camera is null");
  if (prev_transforms && n_prev != r_.scene()->data.transforms.size())
    return bad_argument(err, "motion: the previous transforms must be as many as the scene's (instances index transforms)");
  if (prev.vertices && prev.n_vertices == 0) return bad_argument(err, "motion: previous vertices given, but none of them (n_vertices is 0)");
  if (prev.vertices && (uint64_t)prev.first_vertex + prev.n_vertices > r_.scene()->data.vertices.size())
    return bad_argument(err, "motion: the range of the previous vertices reaches past the scene's vertex count");
  uint32_t posed_first = 0, posed_count = 0;
  if (posed.given) {
    if (prev.vertices) return bad_argument(err, "motion: a posed previous state brings no vertices of its own (vertices must be null)");
    const glz_animation previous = posed.animation();
    if (!r_.scene()->animated_span(&previous, "motion", posed_first, posed_count, err)) return false;
  }
  if (!hip_ok(hipSetDevice(r_.instance()->device), "hipSetDevice", err)) return false;
  MotionStep step;
  host::project_constants(*prev_camera, r_.width(), r_.height(), step.prev.world2camera, step.prev.camera2screen);
  step.prev.persp = prev_camera->type == GLZ_CAMERA_PERSPECTIVE ? 1u : 0u;
  step.prev_o2w = nullptr;
  if (prev_transforms && n_prev > 0) {
    static_assert(sizeof(glz_transform) == 4 * sizeof(float4), "one previous matrix is four float4");
    if (!hip_ok(uploaded.o2w.upload(reinterpret_cast<const float4*>(prev_transforms), 4 * (size_t)n_prev, r_.instance()->stream), "upload previous transforms", err)) return false;
    step.prev_o2w = uploaded.o2w.ptr;
  }
  step.prev_vertices = nullptr;
  step.first_vertex = step.n_vertices = 0;
  if (prev.vertices) {   // as they are: the layout of the scene's own vertices, which the kernel reads for the indices outside the range
    static_assert(sizeof(glz_vertex) == 2 * sizeof(float4), "one vertex is two float4, the position in the first");
    if (!hip_ok(uploaded.vertices.upload(reinterpret_cast<const float4*>(prev.vertices), 2 * (size_t)prev.n_vertices, r_.instance()->stream), "upload previous vertices", err))
      return false;
    step.prev_vertices = uploaded.vertices.ptr;
    step.first_vertex = prev.first_vertex;
    step.n_vertices = prev.n_vertices;
  }
  if (posed.given) {   // the same buffer, filled on the device: the current vertices of the span, then every morph and skin as its previous weights and bones make it
    hipStream_t st = r_.instance()->stream;
    const Scene& scene = *r_.scene();
    if (!hip_ok(uploaded.vertices.alloc(2 * (size_t)posed_count), "alloc previous vertices", err) ||
        !hip_ok(hipMemcpyAsync(uploaded.vertices.ptr, scene.dev.vertices + 2 * (size_t)posed_first, sizeof(float4) * 2 * (size_t)posed_count, hipMemcpyDeviceToDevice, st),
                "copy current vertices", err))
      return false;
    if (!scene.animate_into(posed.animation(), uploaded.vertices.ptr, posed_first, uploaded.animation, st, err)) return false;
    step.prev_vertices = uploaded.vertices.ptr;
    step.first_vertex = posed_first;
    step.n_vertices = posed_count;
  }
  if (!hip_ok(motion.alloc((size_t)r_.width() * r_.height()), "alloc motion plane", err)) return false;
  step.out = motion.ptr;
  step.marks = marks;
  FirstHitRequest pass;
  pass.motion = &step;
  return first_hit_pass(pass, err);
}

bool PostStage::read_motion(const glz_previous_state& prev, float* out, Error& err, const PrevPoses& posed) {
  PrevBuffers uploaded;
  DeviceBuffer<float4> motion;
  if (!motion_pass(prev, uploaded, motion, err, nullptr, posed)) return false;
  return r_.frame_to_host(motion.ptr, out, "read motion", err);
}

bool PostStage::time_motion(const glz_previous_state& prev, float* kernel_ms, Error& err) {
  if (!hip_ok(hipSetDevice(r_.instance()->device), "hipSetDevice", err)) return false;
  Events<2> t;
  PrevBuffers uploaded;
  DeviceBuffer<float4> motion;
  if (!t.create(err) || !motion_pass(prev, uploaded, motion, err, t.ev)) return false;
  if (!hip_ok(hipStreamSynchronize(r_.instance()->stream), "time_motion", err)) return false;
  (void)hipEventElapsedTime(kernel_ms, t.ev[0], t.ev[1]);
  return true;
}

bool PostStage::reproject(const glz_previous_state& prev, const float* prev_color, const float* prev_aov0, const float* prev_aov1, const glz_reproject_params* params,
                          float* out, Error& err, const PrevPoses& posed) {
  const glz_reproject_params P = params ? *params : post::reproject_defaults();
  if (!post::reproject_params_valid(P)) return bad_argument(err, post::kReprojectParamsMessage);
  PrevBuffers uploaded;
  DeviceBuffer<float4> motion, color, plane0, plane1, result;
  if (!motion_pass(prev, uploaded, motion, err, nullptr, posed)) return false;
  const uint32_t w = r_.width(), h = r_.height();
  const size_t n = (size_t)w * h;
  hipStream_t st = r_.instance()->stream;
  if (!hip_ok(color.upload(reinterpret_cast<const float4*>(prev_color), n, st), "upload previous frame", err) ||
      !hip_ok(plane0.upload(reinterpret_cast<const float4*>(prev_aov0), n, st), "upload previous frame", err) ||
      !hip_ok(plane1.upload(reinterpret_cast<const float4*>(prev_aov1), n, st), "upload previous frame", err) || !hip_ok(result.alloc(n), "alloc reprojected frame", err))
    return false;
  if (!hip_ok(launch_reproject(st, w, h, P, motion.ptr, color.ptr, plane0.ptr, plane1.ptr, result.ptr), "k_reproject", err)) return false;
  return r_.frame_to_host(result.ptr, out, "reproject", err);
}

}  // namespace glz
