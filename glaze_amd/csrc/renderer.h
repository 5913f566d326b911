// RayTraceRenderer on HIP (lib/src/vulkan/raytracer.rs:109-687): launch loop, per-launch frame
// constants, accumulation buffers, tile partition for one-process-per-GPU jobs.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <vector>

#include "device_group.h"
#include "host_math.h"
#include "kernels.h"
#include "post_stage.h"
#include "scene.h"
#include "tile_map.h"

namespace glz {

TraceSplitTuning trace_split_from_env();   // renderer.cpp

class Renderer {
 public:
  static Renderer* create(Instance* inst, std::shared_ptr<Scene> scene /* may be null: empty scene */, uint32_t w, uint32_t h, Error& err);
  ~Renderer();

  bool set_integrator(int integrator, Error& err);
  bool set_exposure(float e, Error& err);   // resolves what is pending with the old value first (resolve())
  bool update_camera(const glz_camera& c, Error& err);
  bool change_resolution(uint32_t w, uint32_t h, Error& err);
  bool change_scene(std::shared_ptr<Scene> scene, Error& err);
  bool update_materials_and_lights(const glz_material* m, uint32_t nm, const glz_light* l, uint32_t nl, const glz_texture* t, uint32_t nt, Error& err);
  bool refresh_binded_textures(const glz_texture* t, uint32_t nt, Error& err);
  bool update_transforms(const glz_transform* t, uint32_t n, Error& err);   // Scene::update_transforms; restarts accumulation
  bool update_vertices(const glz_vertex* v, uint32_t first, uint32_t n, int mode, Error& err);   // Scene::update_vertices; restarts accumulation
  int add_skin(const glz_skin& skin, Error& err);       // Scene::add_skin here and on every replica; the id, or -1
  bool remove_skin(int id, Error& err);
  bool set_skin_blend(int id, int blend, Error& err);   // Scene::set_skin_blend here and on every replica
  bool pose_skins(const glz_pose* poses, uint32_t n, int mode, Error& err);   // Scene::pose_skins; restarts accumulation, like update_vertices
  int add_morph(const glz_morph& morph, Error& err);    // Scene::add_morph here and on every replica; the id, or -1
  bool remove_morph(int id, Error& err);
  bool animate(const glz_animation& anim, int mode, Error& err);   // Scene::animate; restarts accumulation, like pose_skins
  // skeletons and clips are the scene's, as skins are: here and on every replica; the id, or -1
  int add_skeleton(const glz_skeleton& skeleton, Error& err);
  bool remove_skeleton(int id, Error& err);
  int add_clip(const glz_clip& clip, Error& err);
  bool remove_clip(int id, Error& err);
  bool play(const glz_play* plays, uint32_t n, int mode, Error& err);   // Scene::play; restarts accumulation, like animate
  int add_normals(const glz_normals& set, Error& err);  // Scene::add_normals here and on every replica; restarts accumulation; the id, or -1
  bool remove_normals(int id, Error& err);
  bool read_vertices(uint32_t first, uint32_t n, glz_vertex* out, Error& err);   // idle first, then the scene's vertices as the device holds them
  bool geometry_update_info(glz_geometry_update_info& out, Error& err);   // Scene::geometry_update_info, idle first (it may make the refit plan); accumulation goes on
  bool wait_idle(Error& err);
  uint32_t steps_per_sample() const { return cfg_.integrator == GLZ_DIRECT ? 1u : cfg_.pt_steps; }

  bool draw(size_t spp, void (*cb)(void*), void* user, uint8_t* rgba8_out, Error& err);
  bool restart();
  bool step(uint32_t n, Error& err);
  bool read_rgba8(uint8_t* out, Error& err);
  bool read_frame(bool result, float* out, Error& err);
  // ---- post (post_stage.h): everything that needs no accumulated frame is called on post() itself; these gather the result first ----
  PostStage& post() { return post_; }
  bool read_denoised(float* rgba32f, uint8_t* rgba8, Error& err) { return read_post(true, rgba32f, rgba8, err); }     // gather + first-hit pass + filter; either output may be null
  bool read_despeckled(float* rgba32f, uint8_t* rgba8, Error& err) { return read_post(false, rgba32f, rgba8, err); }    // gather + first-hit pass + demodulation + rejection; no filter pass
  // one run of the post stages between device events: ms of {first-hit trace, attributes, demodulation, pass 0 .. iterations - 1} (unused = 0)
  bool time_post(float ms[GLZ_POST_TIMING_SLOTS], Error& err);

  bool set_texture_lod(int mode, Error& err);   // 0 = level 0 (the reference), 1 = ray cones; restarts
  bool set_seed(uint64_t s);
  bool set_depth(uint32_t d, Error& err);
  bool set_partition(uint32_t rank, uint32_t world, Error& err);
  // Several GPUs inside ONE process: devices[0] must be this renderer's own device, every further entry renders the
  // tiles t % n == i and every read-out brings them here (device_group.h).  n == 1 returns to a single device.
  bool set_devices(const int* devices, int n, Error& err);
  uint32_t device_count() const { return 1u + (uint32_t)group_.size(); }
  const Scene* device_scene(int i) const { return i == 0 ? scene_.get() : group_.scene(i); }   // the scene (replica) device i of set_devices renders; null when out of range
  bool set_chains(uint32_t n, Error& err);   // 0 = automatic
  // How a launch reaches the device: 1 = two kernels per launch (k_trace, k_shade: throughput, the full frame), 2 = the per-wave
  // launch loop k_path (one kernel per batch of launches: latency, a small tile share per GPU), 0 = by the pixels this device
  // owns.  Images do not depend on it.
  bool set_launch_mode(int mode, Error& err);
  bool path_mode() const { return path_mode_; }
  // Which nodes the two-kernel mode's traversal walks: 4 (k_trace), 8 (k_trace8: flattened scenes, counters off), 0 = by the pixels this device owns.
  bool set_node_width(int width, Error& err);
  bool wide8() const { return wide8_ && !cfg_.counting; }
  uint32_t chains() const { return (uint32_t)chains_.size(); }
  static uint32_t chains_for(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, uint32_t wanted);
  bool export_device(int which, void* dev_rgba32f, Error& err);
  static size_t packed_count(uint32_t w, uint32_t h, uint32_t rank, uint32_t world);   // float4s of a rank's packed tiles
  bool export_packed(int which, void* dev_packed, Error& err);
  bool scatter_packed(uint32_t rank, uint32_t world, const void* dev_packed, void* dev_frame, Error& err);
  bool scatter_packed_all(uint32_t world, const void* dev_packed, uint64_t stride_pixels, void* dev_frame, Error& err);   // every rank's part of one gathered buffer, one synchronisation
  bool tonemap_device(const void* dev_result, uint8_t* out, Error& err);
  bool launch_constants(uint32_t launch, uint32_t* seed, float off[2]);
  void push_constants(float out[32]) const;
  void enable_counters(int flags);
  bool get_stats(glz_render_stats* out, Error& err);

  Instance* instance() const { return inst_; }
  Scene* scene() const { return scene_.get(); }
  uint32_t width() const { return w_; }
  uint32_t height() const { return h_; }
  const CameraConsts& camera_consts() const { return cfg_.cam; }
  bool perspective() const { return cfg_.camera.type == GLZ_CAMERA_PERSPECTIVE; }
  // The tail of every read-out: device arrays to the host on the instance's stream, then the wait for them.  `what` names the read in an error.
  struct HostCopy {
    void* out;
    const void* dev;
    size_t bytes;
  };
  bool to_host(std::initializer_list<HostCopy> copies, const char* what, Error& err) const;
  bool frame_to_host(const float4* frame, void* out, const char* what, Error& err) const { return to_host({{out, frame, sizeof(float4) * (size_t)w_ * h_}}, what, err); }

  // ---- what a DeviceGroup asks of the renderers it drives, beyond the calls above; nothing else uses these ----
  void take_settings(const Renderer& root) { cfg_ = root.cfg_; }                 // a new peer: everything the devices must agree on
  bool set_partition_local(uint32_t rank, uint32_t world, Error& err);           // the tiles t % world == rank, no questions asked
  bool settle(Error& err);                                                       // everything enqueued is done, the images are final
  bool gather(bool result, float4* dst, Error& err, bool zero_first = true);     // every chain's tiles into the full frame `dst`
  struct PackedTiles {
    const TileMap& map;
    const float4* data;   // map.n_local_pixels float4s, tile-major
  };
  PackedTiles packed_tiles(uint32_t chain, bool result) const { return {chains_[chain]->map, result ? chains_[chain]->result.ptr : chains_[chain]->cumulative.ptr}; }

 private:
  Renderer() = default;
  bool allocate(Error& err);
  bool reset_buffers(Error& err);
  bool one_launch(Error& err);
  bool launch_constants_common(FrameData& fd, Error& err);
  bool path_batch(uint32_t n, Error& err);
  bool run_launches(uint32_t n, Error& err);
  bool use_path() const { return path_mode_ && !cfg_.counting && chains_.size() == 1 && chains_[0]->grid_path != 0; }
  template <class A> bool resize(A apply, Error& err);
  template <class U> bool update_scene(U update, Error& err);
  bool rgba8_to_host(const float4* frame, uint8_t* out, const char* what, const char* what_sync, Error& err);

  Instance* inst_ = nullptr;
  std::shared_ptr<Scene> scene_;   // shared with the glz_scene handle it came from (info / debug hooks stay valid)
  uint32_t w_ = 0, h_ = 0;
  // What every device of set_devices must agree on to render one image: a new peer takes it over by one assignment, the setters
  // forward every change.  Deliberately not in here: the partition (rank_, world_: each device has its own), the post stage's
  // parameters and buffers (PostStage: it runs on this device only, on the gathered frame), and everything allocate() derives.
  struct Settings {
    int integrator = GLZ_PATH_TRACE;
    uint32_t pt_steps = 6;   // PT_STEPS, raytrace_structures.rs:87
    int lod_mode = 0;        // texture level of detail: 0 = level 0 always (what the reference's ray-tracing stages do), 1 = ray cones, 2 = ray cones with an anisotropic footprint
    float exposure = 1.0f;
    glz_camera camera{};
    CameraConsts cam{};
    uint64_t seed = 0;
    uint32_t chains_wanted = 0;      // 0 = automatic (pick_chains)
    int launch_mode = getenv("GLAZE_LAUNCH_MODE") ? atoi(getenv("GLAZE_LAUNCH_MODE")) : 0;   // set_launch_mode
    int node_width = getenv("GLAZE_NODE_WIDTH") ? atoi(getenv("GLAZE_NODE_WIDTH")) : 0;   // set_node_width
    bool counting = false;
    bool profile_kernels = true;
    TraceSplitTuning trace_split = trace_split_from_env();   // LaunchArgs::split of every launch: read once, here
  } cfg_;
  host::SeedStream rng_;
  host::WorkScheduler sched_;
  bool request_new_frame_ = true;
  uint32_t rank_ = 0, world_ = 1;   // tile partition of this process (glz_renderer_set_partition)
  bool path_mode_ = false;          // decided in allocate(): this device's launches run as k_path batches
  bool wide8_ = false;              // decided in allocate(): k_trace8 (the 8-wide nodes) traces this device's rays while the counters are off

  // One chain = one independent sequence of launches over a subset of this rank's tiles, on its own HIP stream.
  // Pixels never interact, so the tiles of a rank can advance as several concurrent chains: chain s of S renders the
  // tiles of the finer partition (rank + s * world, world * S).  With few pixels per GPU a launch is bound by the
  // latency of its longest rays, not by throughput; concurrent chains fill the machine during those tails (strong
  // scaling of the 1080p frame over 8 GPUs).  Results are bit-identical for every S.
  struct EventSet {
    hipEvent_t e[4];
    int kind;   // 0: e[0]..e[2] around k_trace, k_shade; 1: e[0]..e[1] around a stand-alone shadow pass; 2: e[0]..e[1] around k_path
    uint32_t weight;   // kind 0: the launches this timed one stands for (event_stride())
  };
  static hipEvent_t last_event(const EventSet& s) { return s.e[s.kind ? 1 : 2]; }
  struct Timed;   // the events around one timed stretch of a chain's stream (renderer.cpp)
  uint64_t event_stride() const;
  struct Chain {
    TileMap map{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DeviceBuffer<float4> ray_o, ray_d, imp[4], hit, sh_o, sh_d, contrib, cumulative, result;
    DeviceBuffer<float> cone;
    DeviceBuffer<uint32_t> hit_inst;
    DeviceBuffer<uint32_t> overflow, queue_count, path_cost;
    uint32_t path_batches = 0;
    uint32_t grid = 0, grid_counting = 0;   // blocks of k_trace's persistent grid (plain / instrumented kernel)
    uint32_t grid8 = 0;                     // ... of k_trace8's (0 unless the renderer walks the 8-wide nodes)
    uint32_t grid_path = 0;                 // blocks of k_path's grid (0: this chain never runs it)
    // shadow rays queued by the last launch's k_shade and not traced yet (they ride in the next launch's k_trace, or in
    // a stand-alone pass as soon as anything looks at the images: flush_shadows)
    bool shadow_pending = false;
    uint32_t pending_set = 0;
    float pending_mark = 0.0f;   // FrameData::update_mark of the launch that queued them
    std::vector<EventSet> pending_events;   // per-launch kernel boundaries, resolved lazily in get_stats
    std::vector<EventSet> free_events;
    double trace_ms = 0, shade_ms = 0, flush_ms = 0, path_ms = 0;
  };
  std::vector<std::unique_ptr<Chain>> chains_;
  uint32_t pick_chains() const;
  uint32_t trace_grid(const Chain& c) const { return cfg_.counting ? c.grid_counting : (wide8() ? c.grid8 : c.grid); }   // blocks of the traversal kernel the chain's launches run
  void release_chains();
  bool flush_shadows(Chain& c, Error& err);
  // The launches write no result and count nothing (accumulate_retired / accumulate_shaded, device/path_state.h); settle() -- every read-out -- and a change of
  // the exposure resolve what they left: the pending shadow rays, then k_finalize on every chain's stream, with the exposure in force
  // for everything it resolves.  The device must be current; nothing waits.
  bool resolve(Error& err);
  float update_mark() const { return -(float)std::min<uint64_t>(accum_launches_, 1u << 24); }   // of the launch counted last
  bool acquire_events(Chain& c, EventSet& ev, Error& err);
  void resolve_events(Chain& c);
  void fill_args(const Chain& c, LaunchArgs& a) const;

  DeviceGroup group_{*this};   // the other GPUs of this process (set_devices)
  bool wait_idle_local(const char* what, Error& err);
  bool step_local(uint32_t n, Error& err);

  bool frame_is_here(const char* who, Error& err) const;                     // false, with the error set, for one rank of a process partition
  // read_denoised (filter) / read_despeckled / time_post (filter, marks: PostStage::filtered's events)
  bool read_post(bool filter, float* rgba32f, uint8_t* rgba8, Error& err, hipEvent_t* marks = nullptr);
  PostStage post_{*this};

  DeviceBuffer<float4> frame_tmp_;
  DeviceBuffer<uchar4> rgba8_;
  DeviceBuffer<float> oetf_thresholds_;   // sRGB8 quantiser thresholds (host::srgb8_thresholds), see k_tonemap
  DeviceBuffer<TraceCounters> counters_;
  uint64_t launches_ = 0;   // stats
  uint64_t accum_launches_ = 0;   // launches since the reset that touched the accumulator (none does in a scene without lights)
  bool resolve_pending_ = false;  // launches have run since the last resolve
};

}  // namespace glz
