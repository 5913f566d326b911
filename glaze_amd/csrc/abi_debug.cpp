// The test hooks of the extern "C" surface (include/glaze_abi.h): the glz_debug_* entry points, which read a scene's device structures
// back or run one kernel on arrays the caller gives, and the glz_host_* ones, which expose host logic that needs no device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "abi_internal.h"
#include "denoise.h"
#include "reproject.h"
#include "skin.h"
#include "clip.h"
#include "morph.h"
#include "normals.h"
#include "mipchain.h"
#include "rccl_dl.h"
#include "tile_map.h"

using namespace glz;
using namespace glz::abi;

namespace {
// One call of a kernel on host arrays.  debug_call sets the device and runs `body`, which launches the kernel and, in doing so, names
// its inputs (uploaded) and outputs (allocated) -- then every output is copied back and the stream synchronised, once.  Every step's
// status is checked: the first that fails ends the call (an Error thrown past what has not run yet) and becomes its status.
struct DebugCall {
  hipStream_t st;
  template <class T>
  const T* in(const T* host, size_t n) {   // a null `host` is an optional input that was not given
    return host ? static_cast<const T*>(buffer(host, n * sizeof(T), nullptr)) : nullptr;
  }
  template <class T>
  T* out(T* host, size_t n) { return static_cast<T*>(buffer(nullptr, n * sizeof(T), host)); }   // a null `host`: scratch, not copied back
  static void check(hipError_t status, const char* what) {
    Error e;
    if (!hip_ok(status, what, e)) throw e;
  }
  struct Buffer { DeviceBuffer<unsigned char> dev; void* host; };
  std::vector<Buffer> buffers;
  void* buffer(const void* upload_from, size_t bytes, void* copy_to) {
    buffers.push_back(Buffer{{}, copy_to});
    DeviceBuffer<unsigned char>& b = buffers.back().dev;
    if (upload_from) check(b.upload(static_cast<const unsigned char*>(upload_from), bytes, st), "debug upload"); else check(b.alloc(bytes), "alloc");
    return b.ptr;
  }
};
template <class Body>
int debug_call(const Instance* inst, const char* what, const char* kernel, Body body) {   // body: hipError_t(DebugCall&)
  try {
    DebugCall::check(hipSetDevice(inst->device), "hipSetDevice");
    DebugCall c{inst->stream};
    DebugCall::check(body(c), kernel);
    for (const DebugCall::Buffer& b : c.buffers)
      if (b.host) DebugCall::check(hipMemcpyAsync(b.host, b.dev.ptr, b.dev.count, hipMemcpyDeviceToHost, c.st), what);
    DebugCall::check(hipStreamSynchronize(c.st), what);
    return GLZ_OK;
  } catch (const Error& e) {
    return fail(e);
  }
}

// the first min(bytes, cap) bytes of one of a scene's device arrays -> out (null: nothing is read); returns `bytes`
int64_t read_array(const Scene& s, const void* dev, size_t bytes, void* out, int64_t cap, const char* what) {
  if (out && cap > 0 && bytes > 0) {
    Error e;
    if (!hip_ok(hipSetDevice(s.instance->device), "hipSetDevice", e)) return fail(e);
    if (!hip_ok(hipMemcpy(out, dev, std::min(bytes, (size_t)cap), hipMemcpyDeviceToHost), what, e)) return fail(e);
  }
  return (int64_t)bytes;
}

// The flattened build links its leaves by NUMBER (the tracer reads one 64-byte BvhQuad per leaf, which names the leaf's first
// triangle slot), and so do the meshes of a two-level scene, by leaf number within the mesh; what the read hooks hand out is the
// structure as its readers walk it -- nodes whose leaf links are ~(first slot in the triangle array) -- so the links are translated.
bool read_quads(const Scene* s, std::vector<BvhQuad>& quads, Error& e) {
  quads.resize(s->accel().n_leaf_records());
  return quads.empty() || hip_ok(hipMemcpy(quads.data(), s->dev.bvh_quads, quads.size() * sizeof(BvhQuad), hipMemcpyDeviceToHost), "read leaf records", e);
}
// nodes [first, last) of an array of `width`-wide nodes whose links start at word `link_offset`; their leaves' records start at quad_base
template <class Node>
void translate_leaf_links(Node* nd, int width, int link_offset, int64_t first, int64_t last, size_t quad_base, const std::vector<BvhQuad>& quads) {
  for (int64_t i = first; i < last; ++i)
    for (int k = 0; k < width; ++k) {
      const int link = (int)nd[i].w[link_offset + k];   // (kBvhEmptyChild is positive)
      if (link < 0 && quad_base + (size_t)~link < quads.size()) nd[i].w[link_offset + k] = (uint32_t)~(int)quads[quad_base + (size_t)~link].slot;
    }
}
}  // namespace

extern "C" {

int glz_debug_post_timing(glz_renderer* h, float ms_out[GLZ_POST_TIMING_SLOTS]) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!ms_out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->time_post(ms_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_camera_rays(glz_renderer* h, float off_x, float off_y, float* origins3, float* dirs3) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!origins3 || !dirs3) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->post().camera_rays(off_x, off_y, origins3, dirs3, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_motion_timing(glz_renderer* h, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev_camera || !kernel_ms_out || prev_camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "bad argument");
  *kernel_ms_out = 0.0f;
  GLZ_RET(h->r->post().time_motion(glz_previous_state{prev_camera, prev_transforms, n_prev_transforms, nullptr, 0, 0}, kernel_ms_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_motion_timing_from(glz_renderer* h, const glz_previous_state* prev, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !kernel_ms_out || prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "bad argument");
  *kernel_ms_out = 0.0f;
  GLZ_RET(h->r->post().time_motion(*prev, kernel_ms_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_skin_timing(glz_renderer* h, const glz_pose* pose, uint32_t reps, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!pose || !kernel_ms_out || !h->r->scene()) return fail(GLZ_E_ARG, "bad argument");
  *kernel_ms_out = 0.0f;
  GLZ_RET(h->r->wait_idle(e) && h->r->scene()->time_skin(*pose, reps, kernel_ms_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_clip_bones(glz_renderer* h, const glz_play* play, float* rows_out, float* weights_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!play || !rows_out || !h->r->scene()) return fail(GLZ_E_ARG, "bad argument");
  GLZ_RET(h->r->wait_idle(e) && h->r->scene()->clip_bones(*play, rows_out, weights_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_clip_timing(glz_renderer* h, const glz_play* plays, uint32_t n_plays, uint32_t reps, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!plays || !kernel_ms_out || !h->r->scene()) return fail(GLZ_E_ARG, "bad argument");
  *kernel_ms_out = 0.0f;
  GLZ_RET(h->r->wait_idle(e) && h->r->scene()->time_clip(plays, n_plays, reps, kernel_ms_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_morph_timing(glz_renderer* h, const glz_animation* one, uint32_t reps, float* kernel_ms_out, uint64_t* bytes_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!one || !kernel_ms_out || !h->r->scene()) return fail(GLZ_E_ARG, "bad argument");
  *kernel_ms_out = 0.0f;
  GLZ_RET(h->r->wait_idle(e) && h->r->scene()->time_morph(*one, reps, kernel_ms_out, bytes_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_normals_timing(glz_renderer* h, int id, uint32_t reps, float ms_out[2], uint64_t bytes_out[2]) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!ms_out || !h->r->scene()) return fail(GLZ_E_ARG, "bad argument");
  ms_out[0] = ms_out[1] = 0.0f;
  GLZ_RET(h->r->wait_idle(e) && h->r->scene()->time_normals(id, reps, ms_out, bytes_out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_guide_chain(glz_renderer* h, uint32_t segment, float* origins3, float* dirs3, uint8_t* alive) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!origins3 || !dirs3 || !alive) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->post().guide_chain(segment, origins3, dirs3, alive, e));
  GLZ_GUARD_END(GLZ_E_IO)
}

int glz_debug_trace_closest(glz_scene* h, const float* o, const float* d, uint64_t n, float tmin, float* t, uint32_t* tri, uint32_t* inst, float* u,
                            float* v) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !o || !d || !t || !tri || !inst || !u || !v) return fail(GLZ_E_ARG, "null argument");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many rays");
  Scene* s = h->s.get();
  return debug_call(s->instance, "debug trace", "k_debug_closest", [&](DebugCall& c) {
    return launch_debug_closest(c.st, s->dev, c.in(o, n * 3), c.in(d, n * 3), (uint32_t)n, tmin, c.out(t, n), c.out(tri, n), c.out(inst, n), c.out(u, n), c.out(v, n),
                                c.out<uint32_t>(nullptr, (n + 512) * s->accel().stack_overflow_depth), s->accel().stack_overflow_depth);
  });
  GLZ_GUARD_END(GLZ_E_IO)
}

int glz_debug_trace_any(glz_scene* h, const float* o, const float* d, const float* tmax, uint64_t n, float tmin, uint8_t* out) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !o || !d || !tmax || !out) return fail(GLZ_E_ARG, "null argument");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many rays");
  Scene* s = h->s.get();
  return debug_call(s->instance, "debug trace", "k_debug_any", [&](DebugCall& c) {
    return launch_debug_any(c.st, s->dev, c.in(o, n * 3), c.in(d, n * 3), c.in(tmax, n), (uint32_t)n, tmin, c.out(out, n),
                            c.out<uint32_t>(nullptr, (n + 512) * s->accel().stack_overflow_depth), s->accel().stack_overflow_depth);
  });
  GLZ_GUARD_END(GLZ_E_IO)
}

int64_t glz_debug_read_derivatives(glz_scene* h, float* out, int64_t cap_tris) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  Scene* s = h->s.get();
  uint32_t ntri = 0;
  for (const glz_mesh& m : s->data.meshes) ntri = std::max<uint32_t>(ntri, (m.index_offset + m.index_count) / 3);
  const int64_t bytes = read_array(*s, s->dev.derivatives, (size_t)ntri * 48, cap_tris > 0 ? out : nullptr, std::min<int64_t>(cap_tris, ntri) * 48, "read derivatives");
  return bytes < 0 ? bytes : ntri;
  GLZ_GUARD_END(GLZ_E_IO)
}
int64_t glz_debug_read_rt_materials(glz_scene* h, void* out, int64_t cap) {
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  return read_array(*h->s, h->s->dev.materials, h->s->tables().h_materials.size() * sizeof(RTMaterial), out, cap, "read materials");
}
int64_t glz_debug_read_rt_lights(glz_scene* h, void* out, int64_t cap) {
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  return read_array(*h->s, h->s->dev.lights, h->s->tables().h_lights.size() * sizeof(RTLight), out, cap, "read lights");
}
int64_t glz_debug_read_sky(glz_scene* h, float* out, int64_t cap) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  Scene* s = h->s.get();
  std::vector<float> buf(36 + 4 + s->tables().h_sky_marginal.size());
  memcpy(buf.data(), &s->tables().h_sky, 144);
  memcpy(buf.data() + 36, &s->tables().h_sky_header, 16);
  if (!s->tables().h_sky_marginal.empty()) {
    Error e;
    if (!hip_ok(hipSetDevice(s->instance->device), "hipSetDevice", e)) return fail(e);
    if (!hip_ok(hipMemcpy(buf.data() + 40, s->dev.sky_marginal, s->tables().h_sky_marginal.size() * 4, hipMemcpyDeviceToHost), "read sky", e)) return fail(e);
  }
  if (out && cap > 0) memcpy(out, buf.data(), (size_t)std::min<int64_t>(cap, (int64_t)buf.size()) * 4);
  return (int64_t)buf.size();
  GLZ_GUARD_END(GLZ_E_IO)
}
int64_t glz_debug_read_bvh(glz_scene* h, void* nodes_out, int64_t cap_nodes, void* tris_out, int64_t cap_tris) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  Scene* s = h->s.get();
  Error e;
  if (!hip_ok(hipSetDevice(s->instance->device), "hipSetDevice", e)) return fail(e);
  const int64_t nn = s->info.bvh_nodes, nt = (int64_t)s->info.n_as_triangles;
  if (nodes_out && cap_nodes > 0 && nn > 0 &&
      !hip_ok(hipMemcpy(nodes_out, s->dev.bvh_nodes, (size_t)std::min(cap_nodes, nn) * sizeof(BvhNode4), hipMemcpyDeviceToHost), "read nodes", e))
    return fail(e);
  if (nodes_out && cap_nodes > 0 && nn > 0 && s->dev.bvh_quads) {
    std::vector<BvhQuad> quads;
    if (!read_quads(s, quads, e)) return fail(e);
    BvhNode4* nd = static_cast<BvhNode4*>(nodes_out);
    const int64_t end = std::min(cap_nodes, nn);
    if (!s->dev.two_level) translate_leaf_links(nd, 4, 12, 0, end, 0, quads);
    else   // the meshes of a two-level scene: leaf number within the mesh -> ~(first slot within the mesh's triangles)
      for (const Accel::MeshRange& m : s->accel().h_mesh_ranges) translate_leaf_links(nd, 4, 12, m.node_base, std::min<int64_t>(end, (int64_t)m.node_base + m.n_nodes), m.quad_base, quads);
  }
  if (tris_out && cap_tris > 0 && nt > 0 &&
      !hip_ok(hipMemcpy(tris_out, s->dev.bvh_tris, (size_t)std::min(cap_tris, nt) * sizeof(BvhTri), hipMemcpyDeviceToHost), "read tris", e))
    return fail(e);
  return nn;
  GLZ_GUARD_END(GLZ_E_IO)
}

int64_t glz_debug_read_tlas_instances(glz_scene* h, void* out, int64_t cap) {
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  return read_array(*h->s, h->s->dev.tlas_instances, h->s->accel().n_tlas_records() * sizeof(TlasInstance), out, cap, "read instance records");
}
static int64_t write_boxes(const std::vector<float4>& lo, const std::vector<float4>& hi, float* lo4, float* hi4) {
  if (lo4 && !lo.empty()) memcpy(lo4, lo.data(), lo.size() * sizeof(float4));
  if (hi4 && !hi.empty()) memcpy(hi4, hi.data(), hi.size() * sizeof(float4));
  return (int64_t)lo.size();
}
int64_t glz_debug_instance_boxes(glz_scene* h, int on_device, uint64_t budget, float* lo4, float* hi4) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  if (!lo4 && !hi4) return (int64_t)(h->s->dev.two_level ? h->s->info.n_instances : 0);   // the count alone, nothing computed
  std::vector<float4> lo, hi;
  Error e;
  if (!h->s->instance_boxes(on_device != 0, budget ? budget : kExactBoxBudget, lo, hi, e) && e.code != GLZ_OK) return fail(e);
  return write_boxes(lo, hi, lo4, hi4);
  GLZ_GUARD_END(GLZ_E_IO)
}
float glz_debug_box_kernel_ms(glz_scene* h) { return h && h->s ? h->s->accel().box_kernel_ms : -1.0f; }
int64_t glz_host_instance_boxes(const glz_scene_desc* d, uint64_t budget, float* lo4, float* hi4) {
  GLZ_GUARD_BEGIN
  if (!d) return fail(GLZ_E_ARG, "scene description is null");
  if ((d->n_vertices && !d->vertices) || (d->n_indices && !d->indices) || (d->n_meshes && !d->meshes) || (d->n_transforms && !d->transforms) ||
      (d->n_instances && !d->instances))
    return fail(GLZ_E_ARG, "null array");
  SceneData data;
  if (d->n_vertices) data.vertices.assign(d->vertices, d->vertices + d->n_vertices);
  if (d->n_indices) data.indices.assign(d->indices, d->indices + d->n_indices);
  if (d->n_meshes) data.meshes.assign(d->meshes, d->meshes + d->n_meshes);
  if (d->n_transforms) data.transforms.assign(d->transforms, d->transforms + d->n_transforms);
  if (d->n_instances) data.instances.assign(d->instances, d->instances + d->n_instances);
  if (!lo4 && !hi4) return (int64_t)rt_instances(data).size();   // the count alone, nothing computed
  std::vector<float4> lo, hi;
  Error e;
  if (!host_instance_boxes_of(data, budget ? budget : kExactBoxBudget, lo, hi, e)) return fail(e);
  return write_boxes(lo, hi, lo4, hi4);
  GLZ_GUARD_END(GLZ_E_IO)
}
int64_t glz_debug_read_bvh8(glz_scene* h, void* nodes_out, int64_t cap_nodes) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  Scene* s = h->s.get();
  Error e;
  if (!hip_ok(hipSetDevice(s->instance->device), "hipSetDevice", e)) return fail(e);
  const int64_t nn = s->dev.bvh_nodes8 ? (int64_t)s->info.bvh_nodes8 : 0;
  if (nodes_out && cap_nodes > 0 && nn > 0) {
    if (!hip_ok(hipMemcpy(nodes_out, s->dev.bvh_nodes8, (size_t)std::min(cap_nodes, nn) * sizeof(BvhNode8), hipMemcpyDeviceToHost), "read 8-wide nodes", e)) return fail(e);
    std::vector<BvhQuad> quads;   // leaf number -> ~(first slot), as glz_debug_read_bvh hands its links out
    if (!read_quads(s, quads, e)) return fail(e);
    translate_leaf_links(static_cast<BvhNode8*>(nodes_out), 8, 24, 0, std::min(cap_nodes, nn), 0, quads);
  }
  return nn;
  GLZ_GUARD_END(GLZ_E_IO)
}

int64_t glz_debug_read_leaf_records(glz_scene* h, void* out, int64_t cap) {
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  const size_t n = h->s->accel().n_leaf_records() - (h->s->dev.two_level && h->s->accel().n_leaf_records() ? 1 : 0);   // (two levels: less the padding record)
  const int64_t bytes = read_array(*h->s, h->s->dev.bvh_quads, n * sizeof(BvhQuad), cap > 0 ? out : nullptr, cap * (int64_t)sizeof(BvhQuad), "read leaf records");
  return bytes < 0 ? bytes : (int64_t)n;
}

int64_t glz_debug_read_texture_level(glz_scene* h, uint32_t texture, uint32_t level, uint8_t* out, int64_t cap, uint32_t* width, uint32_t* height) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s) return fail(GLZ_E_ARG, "scene is null");
  Error e;
  std::vector<uint8_t> px;
  uint32_t w = 0, hh = 0;
  if (!h->s->read_mip_level(texture, level, px, w, hh, e)) return fail(e);
  if (width) *width = w;
  if (height) *height = hh;
  if (out && cap > 0 && !px.empty()) memcpy(out, px.data(), (size_t)std::min<int64_t>(cap, (int64_t)px.size()));
  return (int64_t)px.size();
  GLZ_GUARD_END(GLZ_E_IO)
}
namespace {
// the checks glz_host_denoise and glz_debug_denoise share; returns 0 when there is work to do, 1 for an empty frame
int denoise_arguments(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_denoise_params* p, float* out,
                      glz_denoise_params& P) {
  if (!result || !aov0 || !aov1 || !out) return fail(GLZ_E_ARG, "null argument");
  P = p ? *p : post::denoise_defaults();
  if (!post::denoise_params_valid(P)) return fail(GLZ_E_ARG, post::kDenoiseParamsMessage);
  if ((uint64_t)w * h > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "frame too large");
  return w == 0 || h == 0 ? 1 : 0;
}
}  // namespace
int glz_host_denoise(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_denoise_params* p, float* out) {
  GLZ_GUARD_BEGIN
  glz_denoise_params P;
  const int st = denoise_arguments(w, h, result, aov0, aov1, p, out, P);
  if (st != 0) return st < 0 ? st : GLZ_OK;
  post::host_denoise(w, h, reinterpret_cast<const float4*>(result), reinterpret_cast<const float4*>(aov0), reinterpret_cast<const float4*>(aov1), P,
                     reinterpret_cast<float4*>(out));
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_denoise(glz_instance* inst, uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_denoise_params* p,
                      float* out) {
  GLZ_GUARD_BEGIN
  if (!inst) return fail(GLZ_E_ARG, "null argument");
  glz_denoise_params P;
  const int status = denoise_arguments(w, h, result, aov0, aov1, p, out, P);
  if (status != 0) return status < 0 ? status : GLZ_OK;
  const size_t n = (size_t)w * h;
  return debug_call(inst->i.get(), "debug denoise", "k_atrous", [&](DebugCall& c) {
    return launch_denoise(c.st, w, h, P, c.in(reinterpret_cast<const float4*>(result), n), c.in(reinterpret_cast<const float4*>(aov0), n),
                          c.in(reinterpret_cast<const float4*>(aov1), n), c.out<float4>(nullptr, n), c.out<float4>(nullptr, n), c.out(reinterpret_cast<float4*>(out), n));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
namespace {
// the checks glz_host_despeckle and glz_debug_despeckle share, as denoise_arguments.  Without the filter only eps_albedo of `p` is used, so
// only that is taken from it: the rest of P is the defaults, and a caller's unused fields cannot fail the call
int despeckle_arguments(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_despeckle_params* d,
                        const glz_denoise_params* p, bool with_filter, float* out, glz_despeckle_params& D, glz_denoise_params& P) {
  glz_denoise_params used = post::denoise_defaults();
  if (p && with_filter) used = *p;
  else if (p) used.eps_albedo = p->eps_albedo;
  const int st = denoise_arguments(w, h, result, aov0, aov1, &used, out, P);
  if (st < 0) return st;
  D = d ? *d : post::despeckle_defaults();
  if (!post::despeckle_params_valid(D)) return fail(GLZ_E_ARG, post::kDespeckleParamsMessage);
  return st;
}
}  // namespace
int glz_host_despeckle(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_despeckle_params* d, const glz_denoise_params* p,
                       int with_filter, float* out) {
  GLZ_GUARD_BEGIN
  glz_denoise_params P;
  glz_despeckle_params D;
  const int st = despeckle_arguments(w, h, result, aov0, aov1, d, p, with_filter != 0, out, D, P);
  if (st != 0) return st < 0 ? st : GLZ_OK;
  post::host_despeckle(w, h, reinterpret_cast<const float4*>(result), reinterpret_cast<const float4*>(aov0), reinterpret_cast<const float4*>(aov1), D, P,
                       with_filter != 0, reinterpret_cast<float4*>(out));
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_despeckle(glz_instance* inst, uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1, const glz_despeckle_params* d,
                        const glz_denoise_params* p, int with_filter, float* out, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN
  if (!inst) return fail(GLZ_E_ARG, "null argument");
  glz_denoise_params P;
  glz_despeckle_params D;
  const int status = despeckle_arguments(w, h, result, aov0, aov1, d, p, with_filter != 0, out, D, P);
  if (status < 0) return status;
  if (kernel_ms_out) *kernel_ms_out = 0.0f;
  if (status != 0) return GLZ_OK;
  const size_t n = (size_t)w * h;
  Error e;
  if (!hip_ok(hipSetDevice(inst->i->device), "hipSetDevice", e)) return fail(e);
  Events<2> events;
  if (!events.create(e)) return fail(e);
  hipEvent_t* ev = events.ev;
  const int rc = debug_call(inst->i.get(), "debug despeckle", "k_despeckle", [&](DebugCall& c) {
    const float4* r = c.in(reinterpret_cast<const float4*>(result), n);
    const float4* a0 = c.in(reinterpret_cast<const float4*>(aov0), n);
    const float4* a1 = c.in(reinterpret_cast<const float4*>(aov1), n);
    float4* ping = c.out<float4>(nullptr, n);
    if (with_filter) return launch_denoise(c.st, w, h, P, r, a0, a1, ping, c.out<float4>(nullptr, n), c.out(reinterpret_cast<float4*>(out), n), nullptr, &D, ev);
    return launch_despeckle(c.st, w, h, D, P.eps_albedo, r, a0, a1, ping, c.out(reinterpret_cast<float4*>(out), n), ev);
  });
  if (rc == GLZ_OK && kernel_ms_out) (void)hipEventElapsedTime(kernel_ms_out, ev[0], ev[1]);   // debug_call has synchronised the stream
  return rc;
  GLZ_GUARD_END(GLZ_E_IO)
}
namespace {
// the checks the four projection / reprojection hooks share; 0 = work to do, 1 = nothing to do, negative = a status
int project_arguments(const glz_camera* camera, uint32_t w, uint32_t h, const float* points3, uint64_t n, float* out3, post::ProjectConstants& C) {
  if (!camera || !points3 || !out3 || w == 0 || h == 0 || camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "bad argument");
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many points");
  host::project_constants(*camera, w, h, C.world2camera, C.camera2screen);
  C.persp = camera->type == GLZ_CAMERA_PERSPECTIVE ? 1u : 0u;
  return n == 0 ? 1 : 0;
}
int reproject_arguments(uint32_t w, uint32_t h, const float* motion, const float* color, const float* aov0, const float* aov1, const glz_reproject_params* p, float* out,
                        glz_reproject_params& P) {
  if (!motion || !color || !aov0 || !aov1 || !out) return fail(GLZ_E_ARG, "null argument");
  P = p ? *p : post::reproject_defaults();
  if (!post::reproject_params_valid(P)) return fail(GLZ_E_ARG, post::kReprojectParamsMessage);
  if ((uint64_t)w * h > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "frame too large");
  return w == 0 || h == 0 ? 1 : 0;
}
}  // namespace
int glz_host_project_constants(const glz_camera* camera, uint32_t width, uint32_t height, float out32[32]) {
  if (!camera || !out32 || width == 0 || height == 0 || camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "bad argument");
  host::project_constants(*camera, width, height, out32, out32 + 16);
  return GLZ_OK;
}
int glz_host_project_points(const glz_camera* camera, uint32_t w, uint32_t h, const float* points3, uint64_t n, float* out3) {
  GLZ_GUARD_BEGIN
  post::ProjectConstants C;
  const int st = project_arguments(camera, w, h, points3, n, out3, C);
  if (st != 0) return st < 0 ? st : GLZ_OK;
  post::host_project_points(C, w, h, points3, (size_t)n, out3);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_project_points(glz_instance* inst, const glz_camera* camera, uint32_t w, uint32_t h, const float* points3, uint64_t n, float* out3) {
  GLZ_GUARD_BEGIN
  if (!inst) return fail(GLZ_E_ARG, "null argument");
  post::ProjectConstants C;
  const int st = project_arguments(camera, w, h, points3, n, out3, C);
  if (st != 0) return st < 0 ? st : GLZ_OK;
  return debug_call(inst->i.get(), "debug project points", "k_project_points",
                    [&](DebugCall& c) { return launch_project_points(c.st, C, w, h, c.in(points3, n * 3), (uint32_t)n, c.out(out3, n * 3)); });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_skin(const glz_vertex* bind, const uint16_t* joints, const float* weights, uint64_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out) {
  GLZ_GUARD_BEGIN
  if (n_bones == 0 || !bones) return fail(GLZ_E_ARG, "host_skin: no bones");
  if (n == 0) return GLZ_OK;
  if (!bind || !joints || !weights || !out) return fail(GLZ_E_ARG, "host_skin: null argument");
  for (uint64_t i = 0; i < 4 * n; ++i)
    if (joints[i] >= n_bones) return fail(GLZ_E_ARG, "host_skin: a joint names a bone past n_bones");
  post::host_skin(bind, joints, weights, (size_t)n, bones, n_bones, out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_skin_dq(const glz_vertex* bind, const uint16_t* joints, const float* weights, uint64_t n, const glz_transform* bones, uint32_t n_bones, glz_vertex* out) {
  GLZ_GUARD_BEGIN
  if (n_bones == 0 || !bones) return fail(GLZ_E_ARG, "host_skin_dq: no bones");
  if (n == 0) return GLZ_OK;
  if (!bind || !joints || !weights || !out) return fail(GLZ_E_ARG, "host_skin_dq: null argument");
  for (uint64_t i = 0; i < 4 * n; ++i)
    if (joints[i] >= n_bones) return fail(GLZ_E_ARG, "host_skin_dq: a joint names a bone past n_bones");
  post::host_skin_dq(bind, joints, weights, (size_t)n, bones, n_bones, out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_bone_dual_quats(const glz_transform* bones, uint32_t n, float* out8) {
  GLZ_GUARD_BEGIN
  if (n == 0) return GLZ_OK;
  if (!bones || !out8) return fail(GLZ_E_ARG, "host_bone_dual_quats: null argument");
  for (uint32_t b = 0; b < n; ++b) {
    float4 rows[post::kSkinDqBoneRows];
    post::pack_bone_dq(bones[b], rows);
    memcpy(out8 + 8 * (size_t)b, rows, sizeof rows);
  }
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_clip_bones(const glz_skeleton_desc* skeleton, const glz_clip_desc* clip, float time, glz_transform* bones_out, float* weights_out) {
  GLZ_GUARD_BEGIN
  if (!skeleton || !clip || !bones_out) return fail(GLZ_E_ARG, "host_clip_bones: null argument");
  std::string why;
  if (!post::clip_check_skeleton(skeleton->parents, skeleton->inverse_bind, skeleton->n_bones, why) || !post::clip_check_keys(*clip, why))
    return fail(GLZ_E_ARG, ("host_clip_bones: " + why).c_str());
  if (!std::isfinite(time)) return fail(GLZ_E_ARG, "host_clip_bones: the time is not finite");
  post::host_clip_bones(*skeleton, *clip, time, bones_out, weights_out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_morph(const glz_vertex* base, uint64_t n, const glz_morph_target* targets, uint32_t n_targets, const float* weights, glz_vertex* out) {
  GLZ_GUARD_BEGIN
  if (n_targets == 0 || n_targets > post::kMorphMaxTargets) return fail(GLZ_E_ARG, "host_morph: n_targets must be 1 .. 65536");
  if (n == 0) return GLZ_OK;
  if (!base || !targets || !weights || !out) return fail(GLZ_E_ARG, "host_morph: null argument");
  if (n > 0xFFFFFFFFull) return fail(GLZ_E_ARG, "host_morph: more vertices than a morph can have");
  post::MorphLayout layout;
  std::string why;
  if (!post::pack_morph((uint32_t)n, targets, n_targets, layout, why)) return fail(GLZ_E_ARG, ("host_morph: " + why).c_str());
  post::host_morph(base, layout, weights, out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_vertex_normals(const glz_vertex* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_indices, const glz_mesh* meshes, uint64_t n_meshes,
                            uint32_t first_vertex, uint32_t n, const uint32_t* groups, glz_vertex* out) {
  GLZ_GUARD_BEGIN
  if (!vertices || !out) return fail(GLZ_E_ARG, "host_vertex_normals: null argument");
  post::NormalLayout layout;
  std::string why;
  if (!post::pack_normals(indices, n_indices, meshes, n_meshes, n_vertices, first_vertex, n, groups, layout, why)) return fail(GLZ_E_ARG, ("host_vertex_normals: " + why).c_str());
  post::host_vertex_normals(vertices, layout, out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_weld_groups(const glz_vertex* vertices, uint64_t n, uint32_t* groups_out) {
  GLZ_GUARD_BEGIN
  if (n == 0) return GLZ_OK;
  if (!vertices || !groups_out) return fail(GLZ_E_ARG, "host_weld_groups: null argument");
  if (n > 0xFFFFFFFFull) return fail(GLZ_E_ARG, "host_weld_groups: more vertices than a label can name");
  post::host_weld_groups(vertices, (uint32_t)n, groups_out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_reproject(uint32_t w, uint32_t h, const float* motion, const float* color, const float* aov0, const float* aov1, const glz_reproject_params* p, float* out) {
  GLZ_GUARD_BEGIN
  glz_reproject_params P;
  const int st = reproject_arguments(w, h, motion, color, aov0, aov1, p, out, P);
  if (st != 0) return st < 0 ? st : GLZ_OK;
  post::host_reproject(w, h, reinterpret_cast<const float4*>(motion), reinterpret_cast<const float4*>(color), reinterpret_cast<const float4*>(aov0),
                       reinterpret_cast<const float4*>(aov1), P, reinterpret_cast<float4*>(out));
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_reproject(glz_instance* inst, uint32_t w, uint32_t h, const float* motion, const float* color, const float* aov0, const float* aov1,
                        const glz_reproject_params* p, float* out, float* kernel_ms_out) {
  GLZ_GUARD_BEGIN
  if (!inst) return fail(GLZ_E_ARG, "null argument");
  glz_reproject_params P;
  const int status = reproject_arguments(w, h, motion, color, aov0, aov1, p, out, P);
  if (status < 0) return status;
  if (kernel_ms_out) *kernel_ms_out = 0.0f;
  if (status != 0) return GLZ_OK;
  const size_t n = (size_t)w * h;
  Error e;
  if (!hip_ok(hipSetDevice(inst->i->device), "hipSetDevice", e)) return fail(e);
  Events<2> events;
  if (!events.create(e)) return fail(e);
  hipEvent_t* ev = events.ev;
  const int rc = debug_call(inst->i.get(), "debug reproject", "k_reproject", [&](DebugCall& c) {
    const float4* m = c.in(reinterpret_cast<const float4*>(motion), n);
    const float4* cc = c.in(reinterpret_cast<const float4*>(color), n);
    const float4* a0 = c.in(reinterpret_cast<const float4*>(aov0), n);
    const float4* a1 = c.in(reinterpret_cast<const float4*>(aov1), n);
    return launch_reproject(c.st, w, h, P, m, cc, a0, a1, c.out(reinterpret_cast<float4*>(out), n), ev);
  });
  if (rc == GLZ_OK && kernel_ms_out) (void)hipEventElapsedTime(kernel_ms_out, ev[0], ev[1]);   // debug_call has synchronised the stream
  return rc;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_tonemap(glz_instance* inst, const float* rgba32f, uint64_t n, uint8_t* out) {
  GLZ_GUARD_BEGIN
  if (!inst || !rgba32f || !out) return fail(GLZ_E_ARG, "null argument");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many pixels");
  float thr[256];
  host::srgb8_thresholds(thr);
  return debug_call(inst->i.get(), "debug tonemap", "k_tonemap", [&](DebugCall& c) {
    return launch_tonemap(c.st, (uint32_t)n, c.in(reinterpret_cast<const float4*>(rgba32f), n), c.in(thr, 256), c.out(reinterpret_cast<uchar4*>(out), n));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}

int glz_debug_sample_texture(glz_scene* h, uint32_t texture, const float* uv2, const float* fp4, uint64_t n, float* rgba) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !uv2 || !rgba) return fail(GLZ_E_ARG, "null argument");
  Scene* s = h->s.get();
  if (texture >= s->dev.n_textures) return fail(GLZ_E_ARG, "no such texture");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many coordinates");
  for (uint64_t i = 0; fp4 && i < n; ++i)
    if (!(fp4[4 * i + 3] >= 1.0f && fp4[4 * i + 3] <= 16.0f)) return fail(GLZ_E_ARG, "taps out of 1..16");
  return debug_call(s->instance, "debug sample texture", "k_debug_sample_texture", [&](DebugCall& c) {
    Error e;
    if (fp4 && !s->ensure_mips(e)) throw e;
    return launch_debug_sample_texture(c.st, s->dev, texture, c.in(uv2, n * 2), c.in(fp4, n * 4), (uint32_t)n, c.out(rgba, n * 4));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_detmath(glz_instance* inst, int fn, const float* x, const float* y, float* out, uint64_t n) {
  GLZ_GUARD_BEGIN
  if (!inst || !x || !out || (fn == 3 && !y)) return fail(GLZ_E_ARG, "null argument");
  if (fn < 0 || fn > 5) return fail(GLZ_E_ARG, "no such function");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFFull) return fail(GLZ_E_ARG, "too many values");
  return debug_call(inst->i.get(), "debug detmath", "k_debug_detmath", [&](DebugCall& c) {
    return launch_debug_detmath(c.st, fn, c.in(x, n), c.in(fn == 3 ? y : nullptr, n), (uint32_t)n, c.out(out, n));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_color_to_spec(glz_instance* inst, int illuminant, const float* rgb3, uint64_t n, float* out16) {
  GLZ_GUARD_BEGIN
  if (!inst || !rgb3 || !out16) return fail(GLZ_E_ARG, "null argument");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFull) return fail(GLZ_E_ARG, "too many colours");
  return debug_call(inst->i.get(), "debug color to spectrum", "k_debug_color_to_spec", [&](DebugCall& c) {
    return launch_debug_color_to_spec(c.st, illuminant != 0, c.in(rgb3, n * 3), (uint32_t)n, c.out(out16, n * 16));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_bsdf_value(glz_scene* h, uint32_t material_id, const float* wo3, const float* wi3, const float* uv2, const float* rand1, const float* frame9,
                         uint64_t n, float* value16, float* pdf) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !wo3 || !wi3 || !uv2 || !rand1 || !value16 || !pdf) return fail(GLZ_E_ARG, "null argument");
  Scene* s = h->s.get();
  if (material_id >= s->dev.n_materials) return fail(GLZ_E_ARG, "no such material");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFull) return fail(GLZ_E_ARG, "too many directions");
  return debug_call(s->instance, "debug bsdf value", "k_debug_bsdf_value", [&](DebugCall& c) {
    return launch_debug_bsdf_value(c.st, s->dev, material_id, c.in(wo3, n * 3), c.in(wi3, n * 3), c.in(uv2, 2), c.in(rand1, n), c.in(frame9, 9), (uint32_t)n,
                                   c.out(value16, n * 16), c.out(pdf, n));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_bsdf_sample(glz_scene* h, uint32_t material_id, const float* wo3, const float* uv2, const float* rand3, const float* frame9, uint64_t n,
                          float* wi3, float* value16, float* pdf) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !wo3 || !uv2 || !rand3 || !wi3 || !value16 || !pdf) return fail(GLZ_E_ARG, "null argument");
  Scene* s = h->s.get();
  if (material_id >= s->dev.n_materials) return fail(GLZ_E_ARG, "no such material");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFull) return fail(GLZ_E_ARG, "too many directions");
  return debug_call(s->instance, "debug bsdf sample", "k_debug_bsdf_sample", [&](DebugCall& c) {
    return launch_debug_bsdf_sample(c.st, s->dev, material_id, c.in(wo3, n * 3), c.in(uv2, 2), c.in(rand3, n * 3), c.in(frame9, 9), (uint32_t)n, c.out(wi3, n * 3),
                                    c.out(value16, n * 16), c.out(pdf, n));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_scene_set_spectra(glz_scene* h, uint32_t material_id, const float ior[16], const float ior2abs2[16]) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !ior || !ior2abs2) return fail(GLZ_E_ARG, "null argument");
  Error e;
  GLZ_RET(h->s->debug_set_spectra(material_id, ior, ior2abs2, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_debug_light_sample(glz_scene* h, uint32_t light_index, const float* pos3, const float* rand3, uint64_t n, float scene_radius, float* wi3,
                           float* dist, float* pdf, float* emission16) {
  GLZ_GUARD_BEGIN
  if (!h || !h->s || !pos3 || !rand3 || !wi3 || !dist || !pdf || !emission16) return fail(GLZ_E_ARG, "null argument");
  Scene* s = h->s.get();
  if (light_index >= s->dev.n_rt_lights) return fail(GLZ_E_ARG, "no such light");
  if (n == 0) return GLZ_OK;
  if (n > 0x7FFFFFFull) return fail(GLZ_E_ARG, "too many positions");
  return debug_call(s->instance, "debug light sample", "k_debug_light_sample", [&](DebugCall& c) {
    return launch_debug_light_sample(c.st, s->dev, light_index, c.in(pos3, n * 3), c.in(rand3, n * 3), (uint32_t)n, scene_radius, c.out(wi3, n * 3), c.out(dist, n),
                                     c.out(pdf, n), c.out(emission16, n * 16));
  });
  GLZ_GUARD_END(GLZ_E_IO)
}

int glz_debug_rccl_selftest(glz_instance* inst, uint64_t n, int* version_out) {
  GLZ_GUARD_BEGIN
  if (!inst || n == 0 || n > (1ull << 30)) return fail(GLZ_E_ARG, "bad argument");
  std::string why;
  const Rccl* nc = Rccl::get(why);
  if (!nc) return fail(GLZ_E_DEVICE, why.c_str());
  Error e;
  if (!hip_ok(hipSetDevice(inst->i->device), "hipSetDevice", e)) return fail(e);
  int version = 0;
  (void)nc->GetVersion(&version);
  if (version_out) *version_out = version;
  hipStream_t st = inst->i->stream;
  std::vector<float> host(n), back(n);
  uint32_t x = 12345u;
  for (uint64_t i = 0; i < n; ++i) {   // arbitrary bit patterns that are finite floats
    x = x * 1664525u + 1013904223u;
    const uint32_t bits = (x & 0x807FFFFFu) | (((x >> 23) % 200u + 20u) << 23);
    memcpy(&host[i], &bits, 4);
  }
  DeviceBuffer<float> send, recv;
  if (!hip_ok(send.upload(host.data(), n, st), "upload", e) || !hip_ok(recv.alloc(n), "alloc", e)) return fail(e);
  if (!hip_ok(hipMemsetAsync(recv.ptr, 0, n * 4, st), "memset", e)) return fail(e);
  ncclComm_t comm = nullptr;
  const int dev = inst->i->device;
  ncclResult_t r = nc->CommInitAll(&comm, 1, &dev);
  if (r != ncclSuccess) return fail(GLZ_E_DEVICE, (std::string("ncclCommInitAll: ") + nc->GetErrorString(r)).c_str());
  r = nc->Reduce(send.ptr, recv.ptr, n, ncclFloat, ncclSum, 0, comm, st);
  bool ok = r == ncclSuccess;
  std::string msg = ok ? "" : std::string("ncclReduce: ") + nc->GetErrorString(r);
  if (ok) {
    ok = hip_ok(hipMemcpyAsync(back.data(), recv.ptr, n * 4, hipMemcpyDeviceToHost, st), "read back", e) && hip_ok(hipStreamSynchronize(st), "ncclReduce", e);
    if (!ok) msg = e.msg;
  }
  (void)nc->CommDestroy(comm);
  if (!ok) return fail(GLZ_E_DEVICE, msg.c_str());
  if (memcmp(host.data(), back.data(), n * 4) != 0) return fail(GLZ_E_DEVICE, "ncclReduce on a one-rank communicator changed the data");
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}

// ---- host logic without a device ---------------------------------------------------------------
int glz_host_launch_constants(uint64_t seed, uint32_t launch, uint32_t* seed_out, float offset[2]) {
  GLZ_GUARD_BEGIN
  if (!seed_out || !offset) return fail(GLZ_E_ARG, "output is null");
  if (!host::launch_constants(seed, launch, seed_out, offset)) return fail(GLZ_E_IO, "WorkScheduler::peek disagrees with next()");
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_push_constants(const glz_camera* camera, uint32_t width, uint32_t height, float out32[32]) {
  if (!camera || !out32 || width == 0 || height == 0 || camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "bad argument");
  host::push_constants(*camera, width, height, out32, out32 + 16);
  return GLZ_OK;
}
int glz_host_tile_owner(uint32_t width, uint32_t height, uint32_t world, uint16_t* owner_out) {
  if (!owner_out || world == 0 || world > 65535) return fail(GLZ_E_ARG, "bad argument");
  const TileMap m = make_tile_map(width, height, 0, world);
  for (uint32_t y = 0; y < height; ++y)
    for (uint32_t x = 0; x < width; ++x) owner_out[(size_t)y * width + x] = (uint16_t)tile_owner(tile_of_pixel(m, x, y), world);
  return GLZ_OK;
}
int glz_host_chain_owner(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint32_t chains, uint16_t* owner_out) {
  if (world == 0 || rank >= world || chains > 16 || !width || !height) return fail(GLZ_E_ARG, "bad argument");
  const uint32_t S = Renderer::chains_for(width, height, rank, world, chains);
  const TileMap m = make_tile_map(width, height, rank, world);
  if (owner_out)
    for (uint32_t y = 0; y < height; ++y)
      for (uint32_t x = 0; x < width; ++x) {
        const uint32_t t = tile_of_pixel(m, x, y);
        owner_out[(size_t)y * width + x] = tile_owner(t, world) == rank ? (uint16_t)tile_chain(t, world, S) : (uint16_t)0xFFFF;
      }
  return (int)S;
}

int64_t glz_host_mip_level(const glz_texture* t, uint32_t level, uint8_t* out, int64_t cap, uint32_t* width, uint32_t* height) {
  GLZ_GUARD_BEGIN
  if (!t || !t->pixels || !t->width || !t->height || t->format < 1 || t->format > 3) return fail(GLZ_E_ARG, "bad texture");
  std::vector<host::MipLevel> given(1);
  given[0].width = t->width;
  given[0].height = t->height;
  given[0].pixels.assign(t->pixels, t->pixels + (size_t)t->width * t->height * (t->format == GLZ_TEX_GRAY ? 1 : 4));
  const std::vector<host::MipLevel> chain = host::build_mip_chain(t->format, std::move(given));
  if (level >= chain.size()) {
    if (width) *width = 0;
    if (height) *height = 0;
    return 0;
  }
  const host::MipLevel& m = chain[level];
  if (width) *width = m.width;
  if (height) *height = m.height;
  if (out && cap > 0) memcpy(out, m.pixels.data(), (size_t)std::min<int64_t>(cap, (int64_t)m.pixels.size()));
  return (int64_t)m.pixels.size();
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_host_traversal_offsets_fit(uint64_t n_nodes, uint64_t n_nodes8, uint64_t n_leaves, uint64_t n_instances, uint64_t grid_lanes, uint64_t overflow_depth) {
  const char* what = traversal_offsets_exceeded(TraversalSizes{n_nodes, n_nodes8, n_leaves, n_instances, grid_lanes, overflow_depth});
  return what ? fail(GLZ_E_INVALID_DATA, what) : GLZ_OK;
}
int glz_host_srgb8_thresholds(float thresholds_out[256]) {
  if (!thresholds_out) return fail(GLZ_E_ARG, "output is null");
  host::srgb8_thresholds(thresholds_out);
  return GLZ_OK;
}
int glz_host_sky_row_pairs(const float* marginal_values, const float* conditional_integrals, uint64_t n, float* pairs_out) {
  if (n != 0 && (!marginal_values || !conditional_integrals || !pairs_out)) return fail(GLZ_E_ARG, "glz_host_sky_row_pairs: null array");
  sky_row_pairs(marginal_values, conditional_integrals, (size_t)n, pairs_out);
  return GLZ_OK;
}
int glz_host_sky_bracket_table(const float* cdf, uint64_t size, uint16_t* table_out) {
  if (!table_out || (size != 0 && !cdf) || size > 0xFFFFFFFFull) return fail(GLZ_E_ARG, "glz_host_sky_bracket_table: null array, or a cdf of 2^32 entries");
  sky_bracket_table(cdf, (uint32_t)size, table_out);
  return GLZ_OK;
}
int glz_host_sky_cdf_search(const float* cdf, uint64_t size, const uint16_t* bracket_or_null, const float* xi, uint64_t n, float* sample_out, uint32_t* offset_out) {
  if (size < 2 || size > 0x7FFFFFFFull || !cdf) return fail(GLZ_E_ARG, "glz_host_sky_cdf_search: a cdf has two entries at least");
  if (n != 0 && (!xi || !sample_out || !offset_out)) return fail(GLZ_E_ARG, "glz_host_sky_cdf_search: null array");
  if (bracket_or_null && bracket_or_null[0] != kSkyBracketFallback)   // a table of another cdf must not walk the search out of this one
    for (uint32_t b = 0; b <= kSkyBracketBuckets; ++b)
      if (bracket_or_null[b] > size || (b != 0 && bracket_or_null[b] < bracket_or_null[b - 1])) return fail(GLZ_E_ARG, "glz_host_sky_cdf_search: the bracket table does not fit the cdf");
  for (uint64_t i = 0; i < n; ++i) sample_out[i] = sky_cdf_search(cdf, (uint32_t)size, xi[i], bracket_or_null, &offset_out[i]);
  return GLZ_OK;
}
int glz_host_texel_wrap(const int32_t* i, uint64_t count, int32_t n, int32_t* index_out) {
  if (n <= 0 || (count != 0 && (!i || !index_out))) return fail(GLZ_E_ARG, "glz_host_texel_wrap: a size below 1, or a null array");
  const bool pow2 = (n & (n - 1)) == 0;
  for (uint64_t k = 0; k < count; ++k) {
    const int32_t r = i[k] % n;
    index_out[k] = pow2 ? (i[k] & (n - 1)) : (r < 0 ? r + n : r);
  }
  return GLZ_OK;
}
int glz_host_conductor_finite(const float ior[16], const float ior2abs2[16], int* flag_out) {
  if (!ior || !ior2abs2 || !flag_out) return fail(GLZ_E_ARG, "glz_host_conductor_finite: null argument");
  *flag_out = conductor_finite(ior, ior2abs2) ? 1 : 0;
  return GLZ_OK;
}
int glz_host_metal_spectra(uint32_t metal, float ior_out[16], float ior2abs2_out[16]) {
  if (!ior_out || !ior2abs2_out || !metal_spectra(metal, ior_out, ior2abs2_out)) return fail(GLZ_E_ARG, "glz_host_metal_spectra: no such metal, or a null output");
  return GLZ_OK;
}

}  // extern "C"

int glz_host_build_sah(uint32_t n, const float* box_lo, const float* box_hi, int32_t* children_out, int32_t* parent_out) {
  GLZ_GUARD_BEGIN
  if (n < 2 || !box_lo || !box_hi || !children_out || !parent_out) return fail(GLZ_E_ARG, "glz_host_build_sah: bad argument");
  static_assert(sizeof(float4) == 16 && sizeof(int2) == 8, "layout");
  build_sah_host(n, reinterpret_cast<const float4*>(box_lo), reinterpret_cast<const float4*>(box_hi), reinterpret_cast<int2*>(children_out), parent_out);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
