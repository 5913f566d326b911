// RayTraceRenderer on HIP -- see renderer.h.  Reference: lib/src/vulkan/raytracer.rs.
#include "renderer.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device/tuning.h"

namespace glz {

namespace {
// Kernel boundaries are timed with HIP events on one launch of every `stride` (Renderer::event_stride), at a pseudo-random place
// inside each group of `stride` consecutive launches, and counted `stride` times.  A fixed place would beat against the path depth:
// launch i traces bounce i mod depth of most pixels and the bounces differ in cost.
inline bool timed_launch(uint64_t i /* 1-based */, uint64_t stride) {
  const uint64_t group = (i - 1) / stride;
  uint32_t x = (uint32_t)group * 747796405u + 2891336453u;   // PCG-RXS-M-XS-32
  x = ((x >> ((x >> 28) + 4u)) ^ x) * 277803737u;
  x ^= x >> 22;
  return (i - 1) % stride == x % stride;
}
}
// Three event records around a timed launch cost 5 - 7 us in every chain: 1 % of a full 1080p launch, 5 % of a 1/8 share's (0.130 against
// 0.123 ms per launch with one launch in four timed, tools/timeline_small_share.sh) -- a small share is timed one launch in sixteen.
uint64_t Renderer::event_stride() const {
  uint64_t pixels = 0;
  for (const auto& c : chains_) pixels += c->map.n_local_pixels;
  return pixels >= (1u << 20) ? 4u : 16u;
}

Renderer* Renderer::create(Instance* inst, std::shared_ptr<Scene> scene, uint32_t w, uint32_t h, Error& err) {
  std::unique_ptr<Renderer> r(new Renderer());
  r->inst_ = inst;
  if (!hip_ok(hipSetDevice(inst->device), "hipSetDevice", err)) return nullptr;
  if (!scene) {
    // RayTraceRenderer::new(.., None, ..) renders an empty scene (raytracer.rs:170-174, NoScene)
    SceneData empty;
    empty.camera = default_camera();
    empty.meta = default_meta();
    scene.reset(Scene::create(inst, std::move(empty), err));
    if (!scene) return nullptr;
  }
  r->scene_ = scene;
  if (w == 0 || h == 0) {
    err.fail(GLZ_E_ARG, "resolution must be non-zero");
    return nullptr;
  }
  r->w_ = w;
  r->h_ = h;
  r->cfg_.camera = scene->data.camera;
  r->cfg_.exposure = scene->data.meta.exposure;
  host::push_constants(r->cfg_.camera, w, h, r->cfg_.cam.camera2world, r->cfg_.cam.screen2camera);
  if (!r->allocate(err)) return nullptr;
  return r.release();
}

void Renderer::release_chains() {
  for (auto& c : chains_) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& s : c->pending_events)
      for (auto& e : s.e) (void)hipEventDestroy(e);
    for (auto& s : c->free_events)
      for (auto& e : s.e) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  }
  chains_.clear();
}

Renderer::~Renderer() {
  group_.release();   // the peers first, each on its own device
  if (inst_) (void)hipSetDevice(inst_->device);
  release_chains();
}

// Number of concurrent chains, from the pixels this rank owns (measured on the atrium, ms per launch of one rank's share of
// a 1080p frame with 1 / 2 / 3 chains): 2.07 M pixels 1.29 / 1.36 / 1.42, 1.04 M 0.72 / 0.72 / 0.71, 518 k 0.43 / 0.38 / 0.38,
// 259 k 0.26 / 0.25 / 0.23.  A launch over a million pixels is throughput bound and wants one chain; below that it is bound
// by the latency of its longest rays and concurrent chains fill the machine.  Four chains are slower again: HIP maps streams
// onto GPU_MAX_HW_QUEUES (4) hardware queues and the fourth chain shares one (0.154 -> 0.252 ms for a 1/8 share; with 8 queues
// 0.19 ms, tools/gpu_chain_sweep.py) -- and no number of chains goes below one chain's own step, which lasts as long as its slowest wave.
uint32_t Renderer::chains_for(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t wanted) {
  const TileMap m = make_tile_map(w, h, rank, world);
  const uint32_t local_tiles = m.n_local_tiles;
  const uint64_t pixels = m.n_local_pixels;
  uint32_t want = wanted;
  if (want == 0) want = pixels >= 1000000u ? 1u : (pixels >= 400000u ? 2u : 3u);
  if (want > local_tiles) want = local_tiles;
  return want ? want : 1u;
}
uint32_t Renderer::pick_chains() const { return path_mode_ ? 1u : chains_for(w_, h_, rank_, world_, cfg_.chains_wanted); }

// Automatic launch mode: a device runs its launches as k_path batches only when every 64-pixel group it owns gets a resident wave of its
// own (4 096 on an MI355X at k_path's four waves per SIMD: up to 262 144 pixels) -- with more groups than waves some waves carry two
// groups one after the other and the launch loop loses to the two-kernel mode (a 1/6 share: 0.217 against 0.156 ms per launch) ...
bool Renderer::allocate(Error& err) {
  release_chains();
  {
    const uint64_t pixels = make_tile_map(w_, h_, rank_, world_).n_local_pixels;
    bool fits = false;
    if (cfg_.launch_mode == 0 && pixels > 0 && pixels <= (1u << 22) && scene_->dev.two_level == 0) {
      const uint32_t blocks = (uint32_t)((pixels / 64 + kTraceBlock / 64 - 1) / (kTraceBlock / 64));
      const uint32_t resident = path_resident_blocks(scene_->dev);
      // ... and the launch loop is what pays: where launches are short (a scene of a few thousand triangles: the 512 x 512 cube runs
      // 34 % faster in it, its kernel boundaries were most of a launch) or the chip is less than four fifths full (a 1/16 share of the
      // 1080p atrium: 0.096 against 0.098 ms per launch).  A share that fills every wave slot with a scene of its size is faster as two
      // kernels since round 4 (1080p / 8: 0.129 against 0.134 ms; tools/gpu_partition_timing.py, tools/gpu_batch_length.py).
      fits = resident >= blocks && (scene_->info.n_world_triangles < 4096 || (uint64_t)blocks * 5u <= (uint64_t)resident * 4u);
    }
    path_mode_ = scene_->dev.two_level == 0 && (cfg_.launch_mode == 2 || fits);
    // The two-kernel mode's traversal walks the hierarchy's 8-wide nodes only on request (set_node_width(8), GLAZE_NODE_WIDTH=8): built to
    // shorten a small tile share's chain of dependent node fetches (17.3 against 24.9 visits per sample), measured slower at every share --
    // a 1080p / 8 share 0.140 - 0.145 against 0.1285 ms per launch, / 16 0.098 against 0.097, the full frame 0.93 against 0.79
    // (profiles/r05_wide_nodes.txt): twice the boxes and up to seven conditional pushes make a visit 1.9 x the instructions, and one wave
    // issues them one after the other, so the shorter chain takes as long.
    wide8_ = scene_->dev.two_level == 0 && scene_->dev.bvh_nodes8 != nullptr && cfg_.node_width == 8;
  }
  const uint32_t S = pick_chains();
  const uint32_t od = scene_->accel().stack_overflow_depth;
  for (uint32_t s = 0; s < S; ++s) {
    std::unique_ptr<Chain> c(new Chain());
    if (s == 0) {
      c->stream = inst_->stream;   // glz_instance_stream keeps naming a stream the renderer works on
    } else {
      if (!hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate", err)) return false;
      c->own_stream = true;
    }
    const TileMap& m = c->map = make_chain_map(w_, h_, rank_, world_, s, S);
    const size_t n = m.n_local_pixels;
    // shadow-ray queue: 8 shards of ceil(blocks/8)*256 entries (kernels_render.hip, queue_capacity)
    const size_t n_queue = (((n + 255) / 256 + 7) / 8) * 256 * 8;
    DeviceBuffer<float4>* bufs[] = {&c->ray_o, &c->ray_d, &c->imp[0], &c->imp[1], &c->imp[2], &c->imp[3], &c->hit, &c->sh_o, &c->sh_d, &c->contrib,
                                    &c->cumulative, &c->result};
    for (auto* b : bufs)
      if (!hip_ok(b->alloc((b == &c->sh_o || b == &c->sh_d || b == &c->contrib) ? n_queue : n), "alloc path state", err)) return false;
    if (!hip_ok(c->cone.alloc(n), "alloc path state", err)) return false;
    if (!hip_ok(c->hit_inst.alloc(n), "alloc path state", err)) return false;
    c->grid = trace_grid_blocks(m.n_local_pixels, false, scene_->dev.two_level != 0);
    c->grid_counting = trace_grid_blocks(m.n_local_pixels, true, scene_->dev.two_level != 0);
    c->grid8 = wide8_ ? trace_grid_blocks(m.n_local_pixels, false, false, true) : 0u;
    c->grid_path = path_mode_ ? path_grid_blocks(m.n_local_pixels, scene_->dev) : 0u;
    // traversal spill: one slot of `od` entries per lane of the largest of the persistent grids
    if (!hip_ok(c->overflow.alloc((size_t)std::max(std::max(std::max(c->grid, c->grid_counting), c->grid_path), c->grid8) * kTraceBlock * od), "alloc traversal spill", err)) return false;
    if (!hip_ok(c->queue_count.alloc(kQueueCountWords), "alloc queue counters", err)) return false;
    if (!hip_ok(c->path_cost.alloc(8 + n / 64 + 1), "alloc path costs", err)) return false;
    if (!hip_ok(hipMemsetAsync(c->path_cost.ptr, 0, sizeof(uint32_t) * (8 + n / 64 + 1), c->stream), "clear path costs", err)) return false;
    chains_.push_back(std::move(c));
  }
  if (!hip_ok(frame_tmp_.alloc((size_t)w_ * h_), "alloc frame", err)) return false;
  if (!hip_ok(rgba8_.alloc((size_t)w_ * h_), "alloc rgba8", err)) return false;
  if (!oetf_thresholds_.ptr) {
    float thr[256];
    host::srgb8_thresholds(thr);
    if (!hip_ok(oetf_thresholds_.upload(thr, 256, chains_[0]->stream), "upload OETF thresholds", err)) return false;
    if (!hip_ok(hipStreamSynchronize(chains_[0]->stream), "upload OETF thresholds", err)) return false;   // thr[] is on this stack frame
  }
  if (!hip_ok(counters_.alloc(1), "alloc counters", err)) return false;
  request_new_frame_ = true;
  return true;
}

// the fill_buffer / clear_color_image of a new frame (raytracer.rs:506-532) + scheduler rewind (:483-485)
bool Renderer::reset_buffers(Error& err) {
  // work of the abandoned frame may still be running on the chains' streams
  for (auto& c : chains_)
    if (!hip_ok(hipStreamSynchronize(c->stream), "reset", err)) return false;
  for (auto& cp : chains_) {
    Chain& c = *cp;
    const size_t bytes = sizeof(float4) * (size_t)c.map.n_local_pixels;
    DeviceBuffer<float4>* zero[] = {&c.ray_o, &c.ray_d, &c.imp[0], &c.imp[1], &c.imp[2], &c.imp[3], &c.cumulative, &c.result, &c.contrib};
    for (auto* b : zero)
      if (bytes && !hip_ok(hipMemsetAsync(b->ptr, 0, bytes, c.stream), "clear path state", err)) return false;
    if (!hip_ok(hipMemsetAsync(c.queue_count.ptr, 0, sizeof(uint32_t) * kQueueCountWords, c.stream), "clear queue counters", err)) return false;
    c.shadow_pending = false;   // queued shadow rays of the abandoned frame are dropped with it
    c.trace_ms = c.shade_ms = c.flush_ms = c.path_ms = 0;
    for (auto& s : c.pending_events) c.free_events.push_back(s);
    c.pending_events.clear();
  }
  if (!hip_ok(hipMemsetAsync(counters_.ptr, 0, sizeof(TraceCounters), chains_[0]->stream), "clear counters", err)) return false;
  if (chains_.size() > 1 && !hip_ok(hipStreamSynchronize(chains_[0]->stream), "clear counters", err)) return false;   // the other chains add to them too
  sched_.rewind();
  rng_.reseed(cfg_.seed);   // build-defined: a restart replays the same seed stream (the reference keeps drawing from entropy)
  launches_ = 0;
  accum_launches_ = 0;
  resolve_pending_ = false;   // what the launches of the abandoned frame left is gone with it
  request_new_frame_ = false;
  return true;
}

void Renderer::fill_args(const Chain& c, LaunchArgs& a) const {
  a.scene = scene_->dev;
  a.st.ray_o = c.ray_o.ptr;
  a.st.ray_d = c.ray_d.ptr;
  for (int q = 0; q < 4; ++q) a.st.imp[q] = c.imp[q].ptr;
  a.st.hit = c.hit.ptr;
  a.st.cone = c.cone.ptr;
  a.st.hit_inst = c.hit_inst.ptr;
  a.st.sh_o = c.sh_o.ptr;
  a.st.sh_d = c.sh_d.ptr;
  a.st.contrib = c.contrib.ptr;
  a.st.queue_count = c.queue_count.ptr;
  a.st.cumulative = c.cumulative.ptr;
  a.st.result = c.result.ptr;
  a.st.overflow = c.overflow.ptr;
  a.st.overflow_depth = scene_->accel().stack_overflow_depth;
  a.st.path_cost = c.path_cost.ptr;
  a.map = c.map;
  a.cam = cfg_.cam;
  a.counters = cfg_.counting ? counters_.ptr : nullptr;
  a.do_closest = a.do_shadow = 0;
  a.shade_set = c.pending_set ^ 1u;
  a.shadow_mark = c.pending_mark;
  a.split = cfg_.trace_split;
}

// The defaults of device/tuning.h, or GLAZE_TRACE_SPLIT="<static num>/<den>,<pool num>/<den>,<chunk groups>" (tuning and tests: one
// library serves every setting; the images do not depend on it).  A value that does not parse leaves the defaults.
TraceSplitTuning trace_split_from_env() {
  TraceSplitTuning t{GLZ_TRACE_SPLIT_NUM, GLZ_TRACE_SPLIT_DEN, GLZ_TRACE_POOL_NUM, GLZ_TRACE_POOL_DEN, GLZ_TRACE_POOL_CHUNK};
  unsigned v[5];
  const char* s = getenv("GLAZE_TRACE_SPLIT");
  if (s && sscanf(s, "%u/%u,%u/%u,%u", &v[0], &v[1], &v[2], &v[3], &v[4]) == 5 && v[0] >= 1 && v[1] >= 1 && v[3] >= 1 && v[2] <= v[3] && v[4] >= 1 &&
      v[0] <= 65535 && v[1] <= 65535 && v[3] <= 65535 && v[4] <= 65535)
    t = TraceSplitTuning{v[0], v[1], v[2], v[3], v[4]};
  return t;
}

void Renderer::resolve_events(Chain& c) {
  for (auto& s : c.pending_events) {
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, s.e[0], s.e[1]);
    if (s.kind == 1) {
      c.flush_ms += a;
    } else if (s.kind == 2) {
      c.path_ms += a;
    } else {
      (void)hipEventElapsedTime(&b, s.e[1], s.e[2]);
      const double weight = (double)s.weight;
      c.trace_ms += a * weight;
      c.shade_ms += b * weight;
    }
    c.free_events.push_back(s);
  }
  c.pending_events.clear();
}

bool Renderer::acquire_events(Chain& c, EventSet& ev, Error& err) {
  if (c.free_events.empty()) {
    if (c.pending_events.size() >= 64) {
      // resolve and recycle the pending sets (without the flush get_stats would do)
      if (!hip_ok(hipEventSynchronize(last_event(c.pending_events.back())), "hipEventSynchronize", err)) return false;
      resolve_events(c);
    }
    if (c.free_events.empty()) {
      EventSet fresh{};
      for (auto& e : fresh.e)
        // timing only: without the system-scope fence an event's completion otherwise carries -- the cache write-back and invalidate
        // it costs the kernels that follow (the BVH leaves the L2s at every timed kernel boundary of every chain)
        if (!hip_ok(hipEventCreateWithFlags(&e, hipEventDisableSystemFence), "hipEventCreate", err)) return false;
      c.free_events.push_back(fresh);
    }
  }
  ev = c.free_events.back();
  c.free_events.pop_back();
  return true;
}

// The events around one timed stretch of a chain's stream -- the only place the launch path records events.  begin() with on = false
// makes the other calls no-ops.  On this thread's per-launch path: plain members, nothing allocated but a chain's first event sets.
struct Renderer::Timed {
  Chain& c;
  EventSet ev{};
  bool on = false;
  bool begin(Renderer& r, bool timed, int kind, uint32_t weight, Error& err) {
    on = timed;
    if (!on) return true;
    if (!r.acquire_events(c, ev, err)) return false;
    ev.kind = kind;
    ev.weight = weight;
    (void)hipEventRecord(ev.e[0], c.stream);
    return true;
  }
  void mark() {   // kind 0: between k_trace and k_shade
    if (on) (void)hipEventRecord(ev.e[1], c.stream);
  }
  void end() {
    if (!on) return;
    (void)hipEventRecord(last_event(ev), c.stream);
    c.pending_events.push_back(ev);
  }
};

// Stand-alone shadow pass for the rays the last launch queued: run before anything observes the accumulators.
bool Renderer::flush_shadows(Chain& c, Error& err) {
  if (!c.shadow_pending) return true;
  LaunchArgs a;
  fill_args(c, a);
  memset(&a.frame, 0, sizeof(a.frame));
  a.do_shadow = 1;
  Timed t{c};
  if (!t.begin(*this, cfg_.profile_kernels, 1, 0, err)) return false;
  if (!hip_ok(launch_trace(c.stream, a, trace_grid(c), wide8()), "k_trace (shadow pass)", err)) return false;
  t.end();
  c.shadow_pending = false;
  return true;
}

bool Renderer::resolve(Error& err) {
  if (!resolve_pending_) return true;
  for (auto& cp : chains_) {
    Chain& c = *cp;
    if (!flush_shadows(c, err)) return false;
    if (!hip_ok(launch_finalize(c.stream, c.map, c.cumulative.ptr, c.result.ptr, cfg_.exposure, -update_mark()), "k_finalize", err)) return false;
  }
  resolve_pending_ = false;
  return true;
}

// What one_launch and path_batch start with: a pending restart, then what all launches of a frame share in RTFrameData
// (raytracer.rs:369-613); seed, pixel offset and update mark are per launch
bool Renderer::launch_constants_common(FrameData& fd, Error& err) {
  if (request_new_frame_ && !reset_buffers(err)) return false;
  memset(&fd, 0, sizeof(fd));
  fd.lights_no = scene_->tables().lights_no;
  fd.scene_radius = scene_->data.meta.scene_radius;
  fd.scene_size[0] = (float)w_;
  fd.scene_size[1] = (float)h_;
  for (int k = 0; k < 3; ++k) fd.scene_centre[k] = scene_->data.meta.scene_centre[k];
  fd.camera_persp = cfg_.camera.type == GLZ_CAMERA_PERSPECTIVE ? 1u : 0u;
  fd.pt_steps = cfg_.pt_steps;
  fd.direct_only = cfg_.integrator == GLZ_DIRECT ? 1u : 0u;
  fd.lod_mode = (uint32_t)cfg_.lod_mode;
  if (cfg_.lod_mode != 0) {
    // one pixel of the image plane at unit distance (perspective: the cone's spread) or in world units (orthographic: the
    // cone's constant width), from the projection's vertical scale: screen2camera[1][1] = -tan(fovy / 2) or -scale
    const float pixel = 2.0f * fabsf(cfg_.cam.screen2camera[5]) / (float)h_;
    const bool persp = cfg_.camera.type == GLZ_CAMERA_PERSPECTIVE;
    fd.cone_spread = persp ? pixel : 0.0f;
    fd.cone_width0 = persp ? 0.0f : pixel;
    if (!scene_->mips_ready() && !scene_->ensure_mips(err)) return false;
  }
  fd.pregen = fd.direct_only ? 0u : 1u;
  return true;
}

// draw_frame (raytracer.rs:369-613): one path segment per pixel
bool Renderer::one_launch(Error& err) {
  FrameData fd;
  if (!launch_constants_common(fd, err)) return false;
  fd.seed = rng_.next();                  // rng.gen::<u32>(), raytracer.rs:487
  sched_.next(fd.pixel_offset);           // WorkScheduler::next(), :489
  // the launch after this one, for the paths that end in this one (shade_pixel): anything that could make the next launch differ from
  // what is assumed here -- a new camera, resolution, scene, integrator, a restart -- resets the path state before it runs (reset_buffers)
  sched_.peek(fd.next_pixel_offset);
  ++launches_;
  if (fd.lights_no == 0) return true;   // the raygen shader returns before touching anything (path_trace.rgen:137-141)
  ++accum_launches_;
  resolve_pending_ = true;
  fd.update_mark = update_mark();
  for (auto& cp : chains_) {
    Chain& c = *cp;
    hipStream_t st = c.stream;
    LaunchArgs a;
    fill_args(c, a);
    a.frame = fd;
    a.do_closest = 1;
    a.do_shadow = c.shadow_pending ? 1u : 0u;   // the previous launch's shadow rays ride in this launch's traversal kernel
    const uint64_t stride = event_stride();
    Timed t{c};
    if (!t.begin(*this, cfg_.profile_kernels && timed_launch(launches_, stride), 0, (uint32_t)stride, err)) return false;
    if (!hip_ok(launch_trace(st, a, trace_grid(c), wide8()), "k_trace", err)) return false;
    t.mark();
    if (!hip_ok(launch_shade(st, a), "k_shade", err)) return false;
    t.end();
    c.shadow_pending = true;
    c.pending_set = a.shade_set;
    c.pending_mark = fd.update_mark;
  }
  return true;
}

// n <= kPathMaxLaunches launches of draw_frame in ONE kernel (k_path): the same per-launch constants, in the same order
bool Renderer::path_batch(uint32_t n, Error& err) {
  FrameData fd;
  if (!launch_constants_common(fd, err)) return false;
  PathBatch b;
  memset(&b, 0, sizeof(b));
  b.n = n;
  b.parity = chains_[0]->path_batches++ & 1u;
  for (uint32_t i = 0; i < n; ++i) {
    b.seed[i] = rng_.next();           // rng.gen::<u32>(), raytracer.rs:487
    sched_.next(b.offset[i]);          // WorkScheduler::next(), :489
  }
  sched_.peek(b.offset[n]);            // the launch after the batch (FrameData::next_pixel_offset of its last launch)
  launches_ += n;
  if (fd.lights_no == 0) return true;   // the raygen shader returns before touching anything (path_trace.rgen:137-141)
  b.base_ordinal = (uint32_t)std::min<uint64_t>(accum_launches_, 1u << 24);   // (update_mark sticks there)
  accum_launches_ += n;
  resolve_pending_ = true;
  Chain& c = *chains_[0];
  if (!flush_shadows(c, err)) return false;   // left by launches that ran as two kernels (work counters had been on)
  LaunchArgs a;
  fill_args(c, a);
  a.frame = fd;
  a.counters = nullptr;
  Timed t{c};
  if (!t.begin(*this, cfg_.profile_kernels, 2, 0, err)) return false;
  // the cost accumulator this batch adds to starts empty (the kernel reads the other one, which the batch before filled)
  if (!hip_ok(hipMemsetAsync(c.path_cost.ptr + 4u * b.parity, 0, 16, c.stream), "clear path cost accumulator", err)) return false;
  if (!hip_ok(launch_path(c.stream, a, b, c.grid_path), "k_path", err)) return false;
  t.end();
  return true;   // nothing is pending: the kernel ends with the shadow rays of its last launch
}

bool Renderer::run_launches(uint32_t n, Error& err) {
  while (n != 0) {
    if (use_path()) {
      const uint32_t m = std::min(n, kPathMaxLaunches);
      if (!path_batch(m, err)) return false;
      n -= m;
    } else {
      if (!one_launch(err)) return false;
      --n;
    }
  }
  return true;
}

// A change of something the buffers are sized by: everything enqueued drains, `apply` changes the setting, this device reallocates;
// the caller then has every peer do the same.
template <class A>
bool Renderer::resize(A apply, Error& err) {
  if (!wait_idle(err)) return false;
  apply();
  return allocate(err);
}

bool Renderer::set_launch_mode(int mode, Error& err) {
  if (mode < 0 || mode > 2) return err.fail(GLZ_E_ARG, "launch mode must be 0 (automatic), 1 (two kernels per launch) or 2 (per-wave launch loop)");
  return resize([&] { cfg_.launch_mode = mode; }, err) && group_.forward([=](Renderer& p, Error& e) { return p.set_launch_mode(mode, e); }, err);
}

bool Renderer::set_node_width(int width, Error& err) {
  if (width != 0 && width != 4 && width != 8) return err.fail(GLZ_E_ARG, "node width must be 0 (automatic), 4 or 8");
  return resize([&] { cfg_.node_width = width; }, err) && group_.forward([=](Renderer& p, Error& e) { return p.set_node_width(width, e); }, err);
}

bool Renderer::get_stats(glz_render_stats* out, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  double trace_ms = 0, shade_ms = 0, flush_ms = 0, path_ms = 0;
  for (auto& cp : chains_) {
    Chain& c = *cp;
    if (!flush_shadows(c, err)) return false;   // the counters and timings of the last launch's shadow rays belong to it
    if (!c.pending_events.empty()) {
      if (!hip_ok(hipEventSynchronize(last_event(c.pending_events.back())), "hipEventSynchronize", err)) return false;
      resolve_events(c);
    }
    trace_ms += c.trace_ms;
    shade_ms += c.shade_ms;
    flush_ms += c.flush_ms;
    path_ms += c.path_ms;
  }
  // concurrent chains overlap in time: the mean over chains is the time the rank spent in S concurrent instances of a kernel
  const double inv = chains_.empty() ? 0.0 : 1.0 / (double)chains_.size();
  memset(out, 0, sizeof(*out));
  out->launches = launches_;
  out->samples = owned_pixels(make_tile_map(w_, h_, rank_, world_)) * launches_;
  out->trace_closest_ms = trace_ms * inv;
  out->shade_ms = shade_ms * inv;
  out->trace_shadow_ms = flush_ms * inv;
  out->other_ms = path_ms * inv;   // k_path: the per-wave launch loop of a small tile share (all three phases in one kernel)
  out->render_ms = out->trace_closest_ms + out->shade_ms + out->trace_shadow_ms + out->other_ms;
  for (auto& c : chains_)
    if (!hip_ok(hipStreamSynchronize(c->stream), "read counters", err)) return false;
  TraceCounters c{};
  if (!hip_ok(hipMemcpy(&c, counters_.ptr, sizeof(c), hipMemcpyDeviceToHost), "read counters", err)) return false;
  out->closest_rays = c.closest_rays;
  out->shadow_rays = c.shadow_rays;
  out->closest_nodes = c.closest_nodes;
  out->closest_tris = c.closest_tris;
  out->shadow_nodes = c.shadow_nodes;
  out->shadow_tris = c.shadow_tris;
  out->hits = c.hits;
  out->fresh_paths = c.fresh;
  for (int i = 0; i < 12; ++i) out->phase[i] = c.phase[i];
  out->tex_fetches = c.shade_tex[0] + c.trace_tex[0];
  out->tex_bytes = c.shade_tex[1] + c.trace_tex[1];
  out->alpha_tex_bytes = c.trace_tex[1];
  out->light_samples = c.shade_tex[2];
  out->sky_samples = c.shade_tex[3];
  return group_.add_stats(out, err);
}

void Renderer::enable_counters(int flags) {
  cfg_.counting = (flags & 1) != 0;
  cfg_.profile_kernels = (flags & 2) != 0;
  group_.each([=](Renderer& p) { p.enable_counters(flags); });
}

bool Renderer::set_integrator(int integrator, Error& err) {
  if (integrator != GLZ_DIRECT && integrator != GLZ_PATH_TRACE) return err.fail(GLZ_E_ARG, "unknown integrator");
  if (integrator != cfg_.integrator) {   // raytracer.rs:197
    cfg_.integrator = integrator;
    request_new_frame_ = true;
  }
  return group_.forward([=](Renderer& p, Error& e) { return p.set_integrator(integrator, e); }, err);
}

// raytracer.rs:186-193: no restart.  update_result applies the exposure of the launch that updates the pixel, and a resolve applies one
// exposure to everything it resolves: what is pending is resolved with the old value before the new one holds (stream-ordered, no wait;
// the queued shadow rays belong to launches under the old value and go first).  A frame about to be reset has nothing to keep.
bool Renderer::set_exposure(float e, Error& err) {
  if (e >= 0.0f && e != cfg_.exposure) {
    if (resolve_pending_ && !request_new_frame_ && !(hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err) && resolve(err))) return false;
    cfg_.exposure = e;
  }
  return group_.forward([=](Renderer& p, Error& pe) { return p.set_exposure(e, pe); }, err);   // (it may enqueue: on the peers' own threads)
}

bool Renderer::update_camera(const glz_camera& c, Error& err) {
  if (c.type > GLZ_CAMERA_ORTHOGRAPHIC) return err.fail(GLZ_E_ARG, "unknown camera type");
  cfg_.camera = c;
  host::push_constants(cfg_.camera, w_, h_, cfg_.cam.camera2world, cfg_.cam.screen2camera);
  request_new_frame_ = true;
  const glz_camera cam = c;
  return group_.forward([=](Renderer& p, Error& e) { return p.update_camera(cam, e); }, err);
}

bool Renderer::change_resolution(uint32_t w, uint32_t h, Error& err) {
  if (w == 0 || h == 0) return err.fail(GLZ_E_ARG, "resolution must be non-zero");
  if (!resize([&] {
        w_ = w;
        h_ = h;
        post_.release();
      }, err) || !group_.change_resolution(w, h, err))
    return false;
  return update_camera(cfg_.camera, err);   // raytracer.rs:297
}

bool Renderer::change_scene(std::shared_ptr<Scene> scene, Error& err) {
  if (!scene) return err.fail(GLZ_E_ARG, "scene is null");
  // the other GPUs of this process get replicas of the new scene, in the shape (flattened / two levels) this device built
  if (!resize([&] {
        scene_ = scene;
        cfg_.exposure = scene->data.meta.exposure;
      }, err) || (!group_.empty() && !scene->host_data(err)) || !group_.change_scene(*scene, scene->instance ? *scene->instance : *inst_, err))
    return false;
  return update_camera(scene->data.camera, err);   // raytracer.rs:246-247
}

// An update of the scene object in place, on this device: drained first; the buffers are reallocated only if the update changed what
// allocate() sizes from the scene (the traversal spill's depth, whether there are 8-wide nodes); accumulation restarts.
template <class U>
bool Renderer::update_scene(U update, Error& err) {
  if (!wait_idle(err)) return false;
  const uint32_t od = scene_->accel().stack_overflow_depth;
  const bool wide8 = scene_->dev.bvh_nodes8 != nullptr;
  if (!update()) return false;
  if ((scene_->accel().stack_overflow_depth != od || (scene_->dev.bvh_nodes8 != nullptr) != wide8) && !allocate(err)) return false;
  request_new_frame_ = true;
  return true;
}

bool Renderer::update_materials_and_lights(const glz_material* m, uint32_t nm, const glz_light* l, uint32_t nl, const glz_texture* t, uint32_t nt,
                                           Error& err) {
  if (!update_scene([&] { return scene_->update_materials_and_lights(m, nm, l, nl, t, nt, err); }, err)) return false;   // raytracer.rs:325
  return group_.forward([=](Renderer& p, Error& e) { return p.update_materials_and_lights(m, nm, l, nl, t, nt, e); }, err);
}

// Moves the instances: the scene's structure is rebuilt for the new transforms (the scene object changes, so every renderer that
// shares it sees the move), accumulation restarts, and every other device of set_devices updates its replica the same way.
bool Renderer::update_transforms(const glz_transform* t, uint32_t n, Error& err) {
  if (!update_scene([&] { return scene_->update_transforms(t, n, err); }, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.update_transforms(t, n, e); }, err);
}

// Deforms the meshes: like update_transforms, on the scene object, with a restart, and followed by every other device's replica.
bool Renderer::update_vertices(const glz_vertex* v, uint32_t first, uint32_t n, int mode, Error& err) {
  if (!update_scene([&] { return scene_->update_vertices(v, first, n, mode, err); }, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.update_vertices(v, first, n, mode, e); }, err);
}

// Skins are the scene's: added, removed and posed on the scene object and on every other device's replica, which gives the same ids.
int Renderer::add_skin(const glz_skin& skin, Error& err) {
  if (!wait_idle(err)) return -1;
  const int id = scene_->add_skin(skin, err);
  if (id < 0) return -1;
  const glz_skin k = skin;
  const bool followed = group_.forward([=](Renderer& p, Error& e) {
    const int got = p.add_skin(k, e);
    if (got >= 0 && got != id) e.fail(GLZ_E_DEVICE, "add_skin: a replica gave another skin id");
    return got == id;
  }, err);
  if (!followed) return -1;
  return id;
}
bool Renderer::remove_skin(int id, Error& err) {
  if (!wait_idle(err) || !scene_->remove_skin(id, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.remove_skin(id, e); }, err);
}
// host state alone (the next pose reads it): nothing to wait for, nothing restarts
bool Renderer::set_skin_blend(int id, int blend, Error& err) {
  if (!scene_->set_skin_blend(id, blend, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.set_skin_blend(id, blend, e); }, err);
}
bool Renderer::pose_skins(const glz_pose* poses, uint32_t n, int mode, Error& err) {
  if (!update_scene([&] { return scene_->pose_skins(poses, n, mode, err); }, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.pose_skins(poses, n, mode, e); }, err);
}
// Morphs are the scene's, as skins are.
int Renderer::add_morph(const glz_morph& morph, Error& err) {
  if (!wait_idle(err)) return -1;
  const int id = scene_->add_morph(morph, err);
  if (id < 0) return -1;
  const glz_morph m = morph;
  const bool followed = group_.forward([=](Renderer& p, Error& e) {
    const int got = p.add_morph(m, e);
    if (got >= 0 && got != id) e.fail(GLZ_E_DEVICE, "add_morph: a replica gave another morph id");
    return got == id;
  }, err);
  if (!followed) return -1;
  return id;
}
bool Renderer::remove_morph(int id, Error& err) {
  if (!wait_idle(err) || !scene_->remove_morph(id, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.remove_morph(id, e); }, err);
}
bool Renderer::animate(const glz_animation& anim, int mode, Error& err) {
  if (!update_scene([&] { return scene_->animate(anim, mode, err); }, err)) return false;
  const glz_animation a = anim;
  return group_.forward([=](Renderer& p, Error& e) { return p.animate(a, mode, e); }, err);
}
// Skeletons and clips are the scene's, as skins are.
int Renderer::add_skeleton(const glz_skeleton& skeleton, Error& err) {
  if (!wait_idle(err)) return -1;
  const int id = scene_->add_skeleton(skeleton, err);
  if (id < 0) return -1;
  const glz_skeleton k = skeleton;
  const bool followed = group_.forward([=](Renderer& p, Error& e) {
    const int got = p.add_skeleton(k, e);
    if (got >= 0 && got != id) e.fail(GLZ_E_DEVICE, "add_skeleton: a replica gave another skeleton id");
    return got == id;
  }, err);
  if (!followed) return -1;
  return id;
}
bool Renderer::remove_skeleton(int id, Error& err) {
  if (!wait_idle(err) || !scene_->remove_skeleton(id, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.remove_skeleton(id, e); }, err);
}
int Renderer::add_clip(const glz_clip& clip, Error& err) {
  if (!wait_idle(err)) return -1;
  const int id = scene_->add_clip(clip, err);
  if (id < 0) return -1;
  const glz_clip c = clip;
  const bool followed = group_.forward([=](Renderer& p, Error& e) {
    const int got = p.add_clip(c, e);
    if (got >= 0 && got != id) e.fail(GLZ_E_DEVICE, "add_clip: a replica gave another clip id");
    return got == id;
  }, err);
  if (!followed) return -1;
  return id;
}
bool Renderer::remove_clip(int id, Error& err) {
  if (!wait_idle(err) || !scene_->remove_clip(id, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.remove_clip(id, e); }, err);
}
bool Renderer::play(const glz_play* plays, uint32_t n, int mode, Error& err) {
  if (!update_scene([&] { return scene_->play(plays, n, mode, err); }, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.play(plays, n, mode, e); }, err);
}
// Normal sets are the scene's, as skins and morphs are; adding one changes the vertices' normals, so it is an update of the scene too.
int Renderer::add_normals(const glz_normals& set, Error& err) {
  int id = -1;
  if (!update_scene([&] { return (id = scene_->add_normals(set, err)) >= 0; }, err)) return -1;
  const glz_normals s = set;
  const bool followed = group_.forward([=](Renderer& p, Error& e) {
    const int got = p.add_normals(s, e);
    if (got >= 0 && got != id) e.fail(GLZ_E_DEVICE, "add_normals: a replica gave another id");
    return got == id;
  }, err);
  if (!followed) return -1;
  return id;
}
bool Renderer::remove_normals(int id, Error& err) {
  if (!wait_idle(err) || !scene_->remove_normals(id, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.remove_normals(id, e); }, err);
}
bool Renderer::read_vertices(uint32_t first, uint32_t n, glz_vertex* out, Error& err) {
  return wait_idle(err) && scene_->read_vertices(first, n, out, err);
}

bool Renderer::geometry_update_info(glz_geometry_update_info& out, Error& err) {
  if (!scene_) return err.fail(GLZ_E_ARG, "renderer has no scene");
  return wait_idle(err) && scene_->geometry_update_info(out, err);
}

// raytracer.rs:328-356.  The reference rebuilds descriptors, pipeline and SBT and leaves the accumulation alone; here the
// kernels read the texture array through the scene struct of every launch, so re-uploading it is all there is to do.
bool Renderer::refresh_binded_textures(const glz_texture* t, uint32_t nt, Error& err) {
  if (!wait_idle(err)) return false;
  if (!scene_->refresh_textures(t, nt, err)) return false;
  return group_.forward([=](Renderer& p, Error& e) { return p.refresh_binded_textures(t, nt, e); }, err);
}

// this device's half of wait_idle: the pending shadow rays of every chain go out, then every chain's stream drains
bool Renderer::wait_idle_local(const char* what, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  for (auto& c : chains_)
    if (!flush_shadows(*c, err)) return false;
  for (auto& c : chains_)
    if (!hip_ok(hipStreamSynchronize(c->stream), what, err)) return false;
  return true;
}

bool Renderer::wait_idle(Error& err) {
  return group_.with_peers([](Renderer& p, Error& e) { return p.wait_idle(e); }, [this](Error& e) { return wait_idle_local("wait_idle", e); }, err);
}

bool Renderer::restart() {
  request_new_frame_ = true;
  group_.each([](Renderer& p) { p.restart(); });
  return true;
}

bool Renderer::step_local(uint32_t n, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  return run_launches(n, err);
}

// Every device enqueues the same n launches (same seed stream, same jitter sequence) for its own tiles; the peers' host
// threads work while this thread enqueues the local share.
bool Renderer::step(uint32_t n, Error& err) {
  return group_.with_peers([=](Renderer& p, Error& e) { return p.step_local(n, e); }, [=](Error& e) { return step_local(n, e); }, err);
}

// draw (raytracer.rs:615-687)
bool Renderer::draw(size_t spp, void (*cb)(void*), void* user, uint8_t* rgba8_out, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  restart();
  const size_t steps = steps_per_sample();
  const size_t substep = spp * steps;
  // The launches are enqueued in chunks -- one sample's worth, or as many as one k_path kernel takes (the longer its batch, the less
  // the kernel's slowest wave weighs) -- and the callback fires on this thread once per sample, when the sample's first launch has
  // been enqueued (raytracer.rs:651-653: `if i % steps == 0`); it never said anything about the GPU's progress.
  size_t done = 0, fired = 0;
  while (done < substep) {
    // any device in the per-wave launch loop wants long batches (a root over the residency limit must not hold its peers to one
    // sample per call); with a callback -- a progress bar, a cancel hook -- at most four samples go out between two calls of it
    bool any_path = use_path();
    group_.each([&](Renderer& p) { any_path = any_path || p.use_path(); });
    size_t chunk = any_path ? (size_t)kPathMaxLaunches : steps;
    if (cb && chunk > 4 * steps) chunk = 4 * steps;
    const uint32_t m = (uint32_t)std::min(chunk, substep - done);
    if (!(group_.empty() ? run_launches(m, err) : step(m, err))) return false;
    done += m;
    for (; fired < (done + steps - 1) / steps; ++fired)
      if (cb) cb(user);
  }
  if (spp == 0 && request_new_frame_ && !reset_buffers(err)) return false;
  if (!wait_idle(err)) return false;
  if (rgba8_out) return read_rgba8(rgba8_out, err);
  return true;
}

// every chain scatters its tiles into the full-frame buffer `dst` (the first one clears it); all on the first chain's
// stream after the chains have drained
bool Renderer::gather(bool result, float4* dst, Error& err, bool zero_first) {
  if (!settle(err)) return false;
  hipStream_t st = chains_[0]->stream;
  bool first = zero_first;
  for (auto& c : chains_) {
    if (!hip_ok(launch_export(st, c->map, result ? c->result.ptr : c->cumulative.ptr, dst, first), "k_export", err)) return false;
    first = false;
  }
  return group_.empty() || group_.bring_tiles(result, dst, err);   // the other devices' tiles (device_group.h)
}

// everything this renderer has enqueued is done and its images are final (what gather() establishes before it scatters): cumulative and
// result are resolved here, on this device; every other device of set_devices settles for itself when its tiles are asked for
bool Renderer::settle(Error& err) {
  if (request_new_frame_ && !reset_buffers(err)) return false;
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err) || !resolve(err)) return false;
  return wait_idle(err);
}

// The tails of every read-out, on the instance's stream (the first chain's): device arrays to the host, or a float4 frame through the sRGB8
// quantiser (into rgba8_) to the host; both wait for the copy.  `what` names the read in an error, `what_sync` the wait's.
bool Renderer::to_host(std::initializer_list<HostCopy> copies, const char* what, Error& err) const {
  hipStream_t st = inst_->stream;
  for (const HostCopy& c : copies)
    if (!hip_ok(hipMemcpyAsync(c.out, c.dev, c.bytes, hipMemcpyDeviceToHost, st), what, err)) return false;
  return hip_ok(hipStreamSynchronize(st), what, err);
}
bool Renderer::rgba8_to_host(const float4* frame, uint8_t* out, const char* what, const char* what_sync, Error& err) {
  hipStream_t st = chains_[0]->stream;
  if (!hip_ok(launch_tonemap(st, w_ * h_, frame, oetf_thresholds_.ptr, rgba8_.ptr), "k_tonemap", err)) return false;
  if (!hip_ok(hipMemcpyAsync(out, rgba8_.ptr, (size_t)w_ * h_ * 4, hipMemcpyDeviceToHost, st), what, err)) return false;
  return hip_ok(hipStreamSynchronize(st), what_sync, err);
}

bool Renderer::read_frame(bool result, float* out, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  if (!gather(result, frame_tmp_.ptr, err)) return false;
  return frame_to_host(frame_tmp_.ptr, out, "read frame", err);
}

// blit out32 -> out8 (R8G8B8A8_SRGB) + export (raytracer.rs:576-584, memory.rs:269-483)
bool Renderer::read_rgba8(uint8_t* out, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  if (!gather(true, frame_tmp_.ptr, err)) return false;
  return rgba8_to_host(frame_tmp_.ptr, out, "read rgba8", "read rgba8", err);
}

// ---- post: the reads that need the accumulated frame (everything else is PostStage's own) ------------------------------------------------
// the readers of the whole frame: under set_partition(world > 1) it is not in this process (with set_devices the partition is over this
// process's own devices: gather() brings their tiles)
bool Renderer::frame_is_here(const char* who, Error& err) const {
  if (world_ <= 1 || !group_.empty()) return true;
  return err.fail(GLZ_E_ARG, std::string(who) + ": under set_partition(world > 1) the frame is not in this process");
}

bool Renderer::time_post(float ms[GLZ_POST_TIMING_SLOTS], Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  Events<GLZ_POST_TIMING_SLOTS + 2> t;   // three around the first-hit pass's kernels, 2 + iterations around the filter's
  hipEvent_t* const ev = t.ev;
  if (!t.create(err) || !read_post(true, nullptr, nullptr, err, ev)) return false;
  for (int i = 0; i < GLZ_POST_TIMING_SLOTS; ++i) ms[i] = 0.0f;
  (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
  (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
  for (uint32_t i = 0; i < 1u + post_.denoise().iterations; ++i) (void)hipEventElapsedTime(&ms[2 + i], ev[3 + i], ev[4 + i]);
  return true;
}

// read_denoised (filter: the a-trous passes, with the rejection ahead of them when it is enabled), read_despeckled (the rejection alone) and,
// with marks, time_post: the one place where the accumulated frame meets the stage
bool Renderer::read_post(bool filter, float* rgba32f, uint8_t* rgba8, Error& err, hipEvent_t* marks) {
  const char* what = marks ? "time_post" : filter ? "read denoised" : "read despeckled";
  if (!frame_is_here(marks ? "time_post" : filter ? "read_denoised" : "read_despeckled", err)) return false;
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  if (!gather(true, frame_tmp_.ptr, err)) return false;   // flushes the pending shadow rays, brings the other devices' tiles
  const float4* out = post_.filtered(frame_tmp_.ptr, filter, marks, err);
  if (!out) return false;
  if (rgba32f && !frame_to_host(out, rgba32f, what, err)) return false;
  if (rgba8 && !rgba8_to_host(out, rgba8, what, what, err)) return false;
  return hip_ok(hipStreamSynchronize(inst_->stream), what, err);   // with neither output the filter has still run when this returns
}

bool Renderer::set_texture_lod(int mode, Error& err) {
  if (mode != 0 && mode != 1 && mode != 2) return err.fail(GLZ_E_ARG, "texture LOD mode must be 0 (level 0), 1 (ray cones) or 2 (ray cones, anisotropic footprint)");
  cfg_.lod_mode = mode;
  request_new_frame_ = true;
  return group_.forward([=](Renderer& p, Error& e) { return p.set_texture_lod(mode, e); }, err);
}

bool Renderer::set_seed(uint64_t s) {
  cfg_.seed = s;
  request_new_frame_ = true;
  group_.each([=](Renderer& p) { p.set_seed(s); });
  return true;
}

bool Renderer::set_depth(uint32_t d, Error& err) {
  if (d == 0 || d > 1024) return err.fail(GLZ_E_ARG, "depth (PT_STEPS) must be in 1..1024");
  cfg_.pt_steps = d;
  request_new_frame_ = true;
  bool ok = true;
  group_.each([&](Renderer& p) { ok = ok && p.set_depth(d, err); });
  return ok;
}

bool Renderer::set_partition(uint32_t rank, uint32_t world, Error& err) {
  if (!group_.empty()) return err.fail(GLZ_E_ARG, "a renderer that spans several devices (set_devices) cannot also be one rank of a process partition");
  return set_partition_local(rank, world, err);
}

bool Renderer::set_partition_local(uint32_t rank, uint32_t world, Error& err) {
  if (world == 0 || rank >= world) return err.fail(GLZ_E_ARG, "bad tile partition");
  if (!wait_idle_local("set_partition", err)) return false;
  rank_ = rank;
  world_ = world;
  return allocate(err);
}

// The group checks the list, the environment and RCCL before anything is touched; from the release of the old peers on every failure
// leaves ONE device rendering the whole frame, with a new frame requested.
bool Renderer::set_devices(const int* devices, int n, Error& err) {
  if (world_ != 1 && group_.empty()) return err.fail(GLZ_E_ARG, "set_devices: this renderer is one rank of a process partition (set_partition)");
  DeviceGroup::Plan plan;
  if (!group_.check(devices, n, plan, err)) return false;
  if (!wait_idle(err)) return false;
  group_.release();
  request_new_frame_ = true;
  if (set_partition_local(0, (uint32_t)n, err) && (n == 1 || group_.build(plan, err))) return true;
  group_.release();
  Error ignored;
  (void)set_partition_local(0, 1, ignored);
  return false;
}

bool Renderer::set_chains(uint32_t n, Error& err) {
  if (n > 16) return err.fail(GLZ_E_ARG, "at most 16 chains");
  return resize([&] { cfg_.chains_wanted = n; }, err) && group_.forward([=](Renderer& p, Error& e) { return p.set_chains(n, e); }, err);
}

bool Renderer::export_device(int which, void* dev, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  if (!gather(which != 0, static_cast<float4*>(dev), err)) return false;
  return hip_ok(hipStreamSynchronize(chains_[0]->stream), "export_device", err);
}

// One process per GPU: what a rank hands to the exchange instead of a zero-padded frame -- its tiles only, tile-major, in the
// order of its partition (local tile j = global tile rank + j * world), packed_count() float4s.
size_t Renderer::packed_count(uint32_t w, uint32_t h, uint32_t rank, uint32_t world) {
  if (world == 0 || rank >= world) return 0;
  return make_tile_map(w, h, rank, world).n_local_pixels;
}
bool Renderer::export_packed(int which, void* dev, Error& err) {
  if (!group_.empty()) return err.fail(GLZ_E_ARG, "export_packed is for one rank of a process partition (a renderer that spans devices exchanges by itself)");
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  if (!settle(err)) return false;
  hipStream_t st = chains_[0]->stream;
  const uint32_t S = (uint32_t)chains_.size();
  for (uint32_t s = 0; s < S; ++s) {
    Chain& c = *chains_[s];
    if (!hip_ok(launch_pack_tiles(st, c.map.n_local_pixels, S, s, which ? c.result.ptr : c.cumulative.ptr, static_cast<float4*>(dev)), "k_pack_tiles", err)) return false;
  }
  return hip_ok(hipStreamSynchronize(st), "export_packed", err);
}
// rank 0 of such a job: the packed tiles of partition (rank, world) go to their place in a full frame (nothing else is touched)
bool Renderer::scatter_packed(uint32_t rank, uint32_t world, const void* dev_packed, void* dev_frame, Error& err) {
  if (world == 0 || rank >= world) return err.fail(GLZ_E_ARG, "bad tile partition");
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  hipStream_t st = chains_[0]->stream;
  if (!hip_ok(launch_export(st, make_tile_map(w_, h_, rank, world), static_cast<const float4*>(dev_packed), static_cast<float4*>(dev_frame), false), "k_export (packed tiles)", err)) return false;
  return hip_ok(hipStreamSynchronize(st), "scatter_packed", err);
}

bool Renderer::scatter_packed_all(uint32_t world, const void* dev_packed, uint64_t stride_pixels, void* dev_frame, Error& err) {
  if (world == 0 || stride_pixels < packed_count(w_, h_, 0, world)) return err.fail(GLZ_E_ARG, "scatter_packed_all: the parts must lie at least packed_pixels(0, world) pixels apart");
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  hipStream_t st = chains_[0]->stream;
  for (uint32_t rank = 0; rank < world; ++rank) {
    const TileMap m = make_tile_map(w_, h_, rank, world);
    if (m.n_local_pixels == 0) continue;
    if (!hip_ok(launch_export(st, m, static_cast<const float4*>(dev_packed) + (size_t)rank * stride_pixels, static_cast<float4*>(dev_frame), false), "k_export (packed tiles)", err)) return false;
  }
  return hip_ok(hipStreamSynchronize(st), "scatter_packed_all", err);
}

bool Renderer::tonemap_device(const void* dev_result, uint8_t* out, Error& err) {
  if (!hip_ok(hipSetDevice(inst_->device), "hipSetDevice", err)) return false;
  return rgba8_to_host(static_cast<const float4*>(dev_result), out, "read rgba8", "tonemap_device", err);
}

bool Renderer::launch_constants(uint32_t launch, uint32_t* seed, float off[2]) { return host::launch_constants(cfg_.seed, launch, seed, off); }

void Renderer::push_constants(float out[32]) const {
  memcpy(out, cfg_.cam.camera2world, 64);
  memcpy(out + 16, cfg_.cam.screen2camera, 64);
}

}  // namespace glz
