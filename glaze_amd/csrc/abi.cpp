// extern "C" surface of libglaze_hip.so (include/glaze_abi.h).  Nothing here touches the oracle or
// any CPU rendering path: every render call goes to the HIP kernels or fails with GLZ_E_DEVICE.
#include <cstring>
#include <string>
#include <vector>

#include "abi_internal.h"
#include "serializer.h"
#include "converter.h"
#include "codec/jpeg.h"
#include "codec/png_enc.h"
#include <strings.h>
#include "rccl_dl.h"

using namespace glz;
using namespace glz::abi;

namespace {
thread_local std::string g_error;
thread_local int g_status = GLZ_OK;

template <class T>
int64_t copy_out(const std::vector<T>& v, T* out, int64_t cap) {
  if (out && cap > 0) memcpy(out, v.data(), sizeof(T) * (size_t)std::min<int64_t>(cap, (int64_t)v.size()));
  return (int64_t)v.size();
}
}  // namespace

int glz::abi::fail(const Error& e) {
  g_error = e.msg;
  g_status = e.code == GLZ_OK ? GLZ_E_ARG : e.code;
  return g_status;
}
int glz::abi::fail(int code, const char* msg) {
  g_error = msg;
  g_status = code;
  return code;
}

extern "C" {

const char* glz_last_error(void) { return g_error.c_str(); }
int glz_last_status(void) { return g_status; }
const char* glz_version(void) { return "glaze-hip 0.1 (gfx950)"; }

// ---- parse -----------------------------------------------------------------------------------
glz_parsed* glz_parse(const char* path) {
  GLZ_GUARD_BEGIN
  if (!path) { fail(GLZ_E_ARG, "path is null"); return nullptr; }
  Error e;
  auto p = Parsed::open(path, e);
  if (!p) { fail(e); return nullptr; }
  glz_parsed* h = new glz_parsed();
  h->p = std::move(p);
  return h;
  GLZ_GUARD_END(nullptr)
}
void glz_parsed_free(glz_parsed* h) { delete h; }

#define GLZ_GETTER(NAME, TYPE, CALL)                          \
  int64_t NAME(glz_parsed* h, TYPE* out, int64_t cap) {       \
    GLZ_GUARD_BEGIN                                           \
    if (!h) return fail(GLZ_E_ARG, "parsed handle is null");  \
    Error e;                                                  \
    const std::vector<TYPE>* v = nullptr;                     \
    if (!(CALL)) return fail(e);                              \
    return copy_out(*v, out, cap);                            \
    GLZ_GUARD_END(GLZ_E_IO)                                   \
  }
GLZ_GETTER(glz_parsed_vertices, glz_vertex, h->p->vertices(v, e))
GLZ_GETTER(glz_parsed_transforms, glz_transform, h->p->transforms(v, e))
GLZ_GETTER(glz_parsed_instances, glz_mesh_instance, h->p->instances(v, e))
GLZ_GETTER(glz_parsed_cameras, glz_camera, h->p->cameras(v, e))
GLZ_GETTER(glz_parsed_materials, glz_material, h->p->materials(v, e))
GLZ_GETTER(glz_parsed_lights, glz_light, h->p->lights(v, e))
#undef GLZ_GETTER

int64_t glz_parsed_meshes(glz_parsed* h, glz_mesh* out, int64_t cap) {
  GLZ_GUARD_BEGIN
  if (!h) return fail(GLZ_E_ARG, "parsed handle is null");
  Error e;
  const std::vector<glz_mesh>* m;
  const std::vector<uint32_t>* idx;
  if (!h->p->meshes(m, idx, e)) return fail(e);
  return copy_out(*m, out, cap);
  GLZ_GUARD_END(GLZ_E_IO)
}
int64_t glz_parsed_indices(glz_parsed* h, uint32_t* out, int64_t cap) {
  GLZ_GUARD_BEGIN
  if (!h) return fail(GLZ_E_ARG, "parsed handle is null");
  Error e;
  const std::vector<glz_mesh>* m;
  const std::vector<uint32_t>* idx;
  if (!h->p->meshes(m, idx, e)) return fail(e);
  return copy_out(*idx, out, cap);
  GLZ_GUARD_END(GLZ_E_IO)
}
int64_t glz_parsed_textures(glz_parsed* h, glz_texture* out, int64_t cap) {
  GLZ_GUARD_BEGIN
  if (!h) return fail(GLZ_E_ARG, "parsed handle is null");
  Error e;
  const std::vector<TextureData>* t;
  if (!h->p->textures(t, e)) return fail(e);
  h->tex_view.clear();
  for (const TextureData& td : *t) {
    glz_texture g = td.info;
    g.pixels = td.level0.data();
    h->tex_view.push_back(g);
  }
  return copy_out(h->tex_view, out, cap);
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_parsed_meta(glz_parsed* h, glz_meta* out) {
  GLZ_GUARD_BEGIN
  if (!h || !out) return fail(GLZ_E_ARG, "null argument");
  Error e;
  bool present = false;
  if (!h->p->meta(*out, present, e)) return fail(e);
  return present ? 0 : 1;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_serialize(const char* path, const glz_serialize_desc* d) {
  GLZ_GUARD_BEGIN
  if (!path || !d) return fail(GLZ_E_ARG, "null argument");
  SerializeInput in;
  in.vertices = d->vertices; in.n_vertices = d->n_vertices;
  in.indices = d->indices; in.n_indices = d->n_indices;
  in.meshes = d->meshes; in.n_meshes = d->n_meshes;
  in.transforms = d->transforms; in.n_transforms = d->n_transforms;
  in.instances = d->instances; in.n_instances = d->n_instances;
  in.cameras = d->cameras; in.n_cameras = d->n_cameras;
  in.textures = d->textures; in.n_textures = d->n_textures;
  in.materials = d->materials; in.n_materials = d->n_materials;
  in.lights = d->lights; in.n_lights = d->n_lights;
  in.meta = d->meta;
  Error e;
  if (!serialize_scene(path, in, e)) return fail(e);
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_parsed_update(glz_parsed* h, const glz_camera* cameras, int64_t n_cameras, const glz_material* materials, int64_t n_materials,
                      const glz_light* lights, int64_t n_lights, const glz_texture* textures, int64_t n_textures, const glz_meta* meta) {
  GLZ_GUARD_BEGIN
  if (!h) return fail(GLZ_E_ARG, "parsed handle is null");
  Parsed::Update u;
  u.cameras = cameras; u.n_cameras = n_cameras;
  u.materials = materials; u.n_materials = n_materials;
  u.lights = lights; u.n_lights = n_lights;
  u.textures = textures; u.n_textures = n_textures;
  u.meta = meta;
  Error e;
  if (!h->p->update(u, e)) return fail(e);
  h->tex_view.clear();
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_save_image(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height) {
  GLZ_GUARD_BEGIN
  if (!path || !rgba8 || !width || !height) return fail(GLZ_E_ARG, "null argument or empty image");
  const std::string p(path);
  auto ends = [&](const char* suf) { const size_t n = strlen(suf); return p.size() >= n && strcasecmp(p.c_str() + p.size() - n, suf) == 0; };
  std::vector<uint8_t> bytes;
  bool ok;
  if (ends(".png")) ok = png_encode(rgba8, width, height, 4, bytes);
  else if (ends(".jpg") || ends(".jpeg")) ok = jpeg_encode(rgba8, width, height, 4, 75, bytes);
  else return fail(GLZ_E_INVALID_INPUT, "The output image must end with .jpg or .png");
  if (!ok) return fail(GLZ_E_INVALID_INPUT, "image cannot be encoded (JPEG is limited to 65535 x 65535)");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(GLZ_E_IO, "The output file can not be written");
  ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  ok = (fclose(f) == 0) && ok;
  return ok ? GLZ_OK : fail(GLZ_E_IO, "short write");
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_convert_obj(const char* input_obj, const char* output_glaze, int gen_mipmaps, uint64_t counts[6]) {
  GLZ_GUARD_BEGIN
  if (!input_obj || !output_glaze) return fail(GLZ_E_ARG, "null argument");
  Error e;
  ConvertReport rep;
  if (!convert_obj(input_obj, output_glaze, gen_mipmaps != 0, &rep, e)) return fail(e);
  if (counts) {
    counts[0] = rep.vertices; counts[1] = rep.triangles; counts[2] = rep.meshes;
    counts[3] = rep.materials; counts[4] = rep.textures; counts[5] = rep.lights;
  }
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_converted_file(const char* path) {
  if (!path) return 0;
  FILE* f = fopen(path, "rb");
  if (!f) return 0;
  unsigned char hdr[16];
  size_t n = fread(hdr, 1, 16, f);
  fclose(f);
  return n == 16 && memcmp(hdr, "glaze", 5) == 0;
}

// ---- instance --------------------------------------------------------------------------------
glz_instance* glz_instance_create(int hip_device) {
  GLZ_GUARD_BEGIN
  Error e;
  Instance* i = Instance::create(hip_device, e);
  if (!i) { fail(e); return nullptr; }
  glz_instance* h = new glz_instance();
  h->i.reset(i);
  return h;
  GLZ_GUARD_END(nullptr)
}
void glz_instance_destroy(glz_instance* h) { delete h; }
int glz_instance_device(const glz_instance* h) { return h ? h->i->device : -1; }
void* glz_instance_stream(const glz_instance* h) { return h ? (void*)h->i->stream : nullptr; }
int glz_instance_set_bvh_builder(glz_instance* h, int builder) {
  if (!h || (builder < GLZ_BVH_LBVH || builder > GLZ_BVH_SAH_HOST)) return fail(GLZ_E_INVALID_INPUT, "glz_instance_set_bvh_builder: bad argument");
  h->i->bvh_builder = builder;
  return GLZ_OK;
}

int glz_instance_set_as_levels(glz_instance* h, int mode) {
  if (!h || mode < GLZ_AS_AUTO || mode > GLZ_AS_TWO_LEVEL) return fail(GLZ_E_INVALID_INPUT, "glz_instance_set_as_levels: bad argument");
  h->i->as_levels = mode;
  return GLZ_OK;
}

// ---- scene -----------------------------------------------------------------------------------
glz_scene* glz_scene_create(glz_instance* inst, glz_parsed* parsed) {
  GLZ_GUARD_BEGIN
  if (!inst || !parsed) { fail(GLZ_E_ARG, "null argument"); return nullptr; }
  Error e;
  SceneData data;
  parsed->p->to_scene_data(data, e);
  delete parsed;   // consumed, like the Box moved into RayTraceScene::new
  Scene* s = Scene::create(inst->i.get(), std::move(data), e);
  if (!s) { fail(e); return nullptr; }
  glz_scene* h = new glz_scene();
  h->s.reset(s);
  return h;
  GLZ_GUARD_END(nullptr)
}

glz_scene* glz_scene_create_from_desc(glz_instance* inst, const glz_scene_desc* d) {
  GLZ_GUARD_BEGIN
  if (!inst || !d) { fail(GLZ_E_ARG, "null argument"); return nullptr; }
  SceneData data;
  if (d->n_vertices) data.vertices.assign(d->vertices, d->vertices + d->n_vertices);
  if (d->n_indices) data.indices.assign(d->indices, d->indices + d->n_indices);
  if (d->n_meshes) data.meshes.assign(d->meshes, d->meshes + d->n_meshes);
  if (d->n_transforms) data.transforms.assign(d->transforms, d->transforms + d->n_transforms);
  if (d->n_instances) data.instances.assign(d->instances, d->instances + d->n_instances);
  if (d->n_materials) data.materials.assign(d->materials, d->materials + d->n_materials);
  if (d->n_lights) data.lights.assign(d->lights, d->lights + d->n_lights);
  for (uint32_t i = 0; i < d->n_textures; ++i) {
    const glz_texture& t = d->textures[i];
    if (!t.pixels || t.format < 1 || t.format > 3) { fail(GLZ_E_ARG, "bad texture in scene description"); return nullptr; }
    TextureData td;
    td.info = t;
    const size_t bytes = (size_t)t.width * t.height * (t.format == GLZ_TEX_GRAY ? 1 : 4);
    td.level0.assign(t.pixels, t.pixels + bytes);
    td.info.pixels = nullptr;
    data.textures.push_back(std::move(td));
  }
  data.has_camera = d->camera != nullptr;
  data.camera = d->camera ? *d->camera : default_camera();
  data.has_meta = d->meta != nullptr;
  data.meta = d->meta ? *d->meta : default_meta();
  if (data.camera.type > GLZ_CAMERA_ORTHOGRAPHIC) { fail(GLZ_E_ARG, "unknown camera type"); return nullptr; }
  Error e;
  Scene* s = Scene::create(inst->i.get(), std::move(data), e);
  if (!s) { fail(e); return nullptr; }
  glz_scene* h = new glz_scene();
  h->s.reset(s);
  return h;
  GLZ_GUARD_END(nullptr)
}

void glz_scene_destroy(glz_scene* h) {
  if (!h) return;
  delete h;
}
int glz_scene_get_info(const glz_scene* h, glz_scene_info* out) {
  if (!h || !h->s || !out) return fail(GLZ_E_ARG, "null argument");
  *out = h->s->info;
  return GLZ_OK;
}
int glz_scene_camera(const glz_scene* h, glz_camera* out) {
  if (!h || !h->s || !out) return fail(GLZ_E_ARG, "null argument");
  *out = h->s->data.camera;
  return GLZ_OK;
}

// ---- renderer --------------------------------------------------------------------------------
glz_renderer* glz_renderer_create(glz_instance* inst, glz_scene* scene, uint32_t w, uint32_t h) {
  GLZ_GUARD_BEGIN
  if (!inst) { fail(GLZ_E_ARG, "instance is null"); return nullptr; }
  if (scene && !scene->owned) { fail(GLZ_E_ARG, "scene already belongs to a renderer"); return nullptr; }
  Error e;
  if (scene) scene->owned = false;   // moved into the renderer (raytracer.rs:109-111); the handle stays valid for debug hooks
  Renderer* r = Renderer::create(inst->i.get(), scene ? scene->s : std::shared_ptr<Scene>(), w, h, e);
  if (!r) {
    fail(e);
    return nullptr;
  }
  glz_renderer* hr = new glz_renderer();
  hr->r.reset(r);
  return hr;
  GLZ_GUARD_END(nullptr)
}
void glz_renderer_destroy(glz_renderer* h) { delete h; }



int glz_renderer_set_integrator(glz_renderer* h, int i) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_integrator(i, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_set_exposure(glz_renderer* h, float x) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_exposure(x, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_update_camera(glz_renderer* h, const glz_camera* c) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!c) return fail(GLZ_E_ARG, "camera is null");
  GLZ_RET(h->r->update_camera(*c, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_change_resolution(glz_renderer* h, uint32_t w, uint32_t hh) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->change_resolution(w, hh, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_change_scene(glz_renderer* h, glz_scene* s) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!s || !s->s || !s->owned) return fail(GLZ_E_ARG, "scene is null or already owned by a renderer");
  s->owned = false;
  GLZ_RET(h->r->change_scene(s->s, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_update_materials_and_lights(glz_renderer* h, const glz_material* m, uint32_t nm, const glz_light* l, uint32_t nl,
                                             const glz_texture* t, uint32_t nt) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if ((!m && nm) || (!l && nl) || (t && !nt)) return fail(GLZ_E_ARG, "null array");
  GLZ_RET(h->r->update_materials_and_lights(m, nm, l, nl, t, nt, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_update_transforms(glz_renderer* h, const glz_transform* t, uint32_t nt) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!t) return fail(GLZ_E_ARG, "transforms is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  if (nt != h->r->scene()->data.transforms.size()) return fail(GLZ_E_ARG, "update_transforms: the transform count must not change (instances index transforms)");
  GLZ_RET(h->r->update_transforms(t, nt, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_update_vertices(glz_renderer* h, const glz_vertex* v, uint32_t first, uint32_t n, int mode) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!v || !n) return fail(GLZ_E_ARG, "update_vertices: vertices is null or empty");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  if ((uint64_t)first + n > h->r->scene()->data.vertices.size()) return fail(GLZ_E_ARG, "update_vertices: the range reaches past the scene's vertex count");
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return fail(GLZ_E_ARG, "update_vertices: unknown mode");
  GLZ_RET(h->r->update_vertices(v, first, n, mode, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_geometry_update_info(glz_renderer* h, glz_geometry_update_info* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->geometry_update_info(*out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_add_skin(glz_renderer* h, const glz_skin* skin) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!skin) return fail(GLZ_E_ARG, "add_skin: the skin is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int id = h->r->add_skin(*skin, e);
  if (id < 0) return fail(e);
  return id;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_remove_skin(glz_renderer* h, int skin) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->remove_skin(skin, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_set_skin_blend(glz_renderer* h, int skin, int blend) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->set_skin_blend(skin, blend, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_skin_blend(glz_renderer* h, int skin) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int blend = h->r->scene()->skin_blend(skin, e);
  if (blend < 0) return fail(e);
  return blend;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_pose_skins(glz_renderer* h, const glz_pose* poses, uint32_t n, int mode) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  // (checked here as well as in the scene: a refused call must not make the renderer drain and restart)
  uint32_t first = 0, count = 0;
  const glz_animation posed{nullptr, 0, poses, n};
  if (!h->r->scene()->animated_span(&posed, "pose_skins", first, count, e)) return fail(e);
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return fail(GLZ_E_ARG, "pose_skins: unknown mode");
  GLZ_RET(h->r->pose_skins(poses, n, mode, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_add_morph(glz_renderer* h, const glz_morph* morph) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!morph) return fail(GLZ_E_ARG, "add_morph: the morph is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int id = h->r->add_morph(*morph, e);
  if (id < 0) return fail(e);
  return id;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_remove_morph(glz_renderer* h, int morph) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->remove_morph(morph, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_animate(glz_renderer* h, const glz_animation* anim, int mode) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  // (checked here as well as in the scene: a refused call must not make the renderer drain and restart)
  uint32_t first = 0, count = 0;
  if (!h->r->scene()->animated_span(anim, "animate", first, count, e)) return fail(e);
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return fail(GLZ_E_ARG, "animate: unknown mode");
  GLZ_RET(h->r->animate(*anim, mode, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_add_skeleton(glz_renderer* h, const glz_skeleton* skeleton) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!skeleton) return fail(GLZ_E_ARG, "add_skeleton: the skeleton is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int id = h->r->add_skeleton(*skeleton, e);
  if (id < 0) return fail(e);
  return id;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_remove_skeleton(glz_renderer* h, int skeleton) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->remove_skeleton(skeleton, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_add_clip(glz_renderer* h, const glz_clip* clip) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!clip) return fail(GLZ_E_ARG, "add_clip: the clip is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int id = h->r->add_clip(*clip, e);
  if (id < 0) return fail(e);
  return id;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_remove_clip(glz_renderer* h, int clip) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->remove_clip(clip, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_play(glz_renderer* h, const glz_play* plays, uint32_t n, int mode) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  // (checked here as well as in the scene: a refused call must not make the renderer drain and restart)
  uint32_t first = 0, count = 0;
  if (!h->r->scene()->played_span(plays, n, "play", first, count, e)) return fail(e);
  if (mode != GLZ_GEOMETRY_REFIT && mode != GLZ_GEOMETRY_REBUILD) return fail(GLZ_E_ARG, "play: unknown mode");
  GLZ_RET(h->r->play(plays, n, mode, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_add_normals(glz_renderer* h, const glz_normals* set) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!set) return fail(GLZ_E_ARG, "add_normals: the set is null");
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  const int id = h->r->add_normals(*set, e);
  if (id < 0) return fail(e);
  return id;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_remove_normals(glz_renderer* h, int id) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  GLZ_RET(h->r->remove_normals(id, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_vertices(glz_renderer* h, uint32_t first, uint32_t n, glz_vertex* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!h->r->scene()) return fail(GLZ_E_ARG, "renderer has no scene");
  if (!out || !n || (uint64_t)first + n > h->r->scene()->data.vertices.size()) return fail(GLZ_E_ARG, "read_vertices: null output, none, or a range past the scene's vertex count");
  GLZ_RET(h->r->read_vertices(first, n, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_refresh_binded_textures(glz_renderer* h, const glz_texture* t, uint32_t nt) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!t || !nt) return fail(GLZ_E_ARG, "null array");
  GLZ_RET(h->r->refresh_binded_textures(t, nt, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_wait_idle(glz_renderer* h) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->wait_idle(e)); GLZ_GUARD_END(GLZ_E_IO) }
uint32_t glz_renderer_steps_per_sample(const glz_renderer* h) { return h ? h->r->steps_per_sample() : 0; }
int glz_renderer_draw(glz_renderer* h, size_t spp, void (*cb)(void*), void* user, uint8_t* out) {
  GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->draw(spp, cb, user, out, e)); GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_restart(glz_renderer* h) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->restart()); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_step(glz_renderer* h, uint32_t n) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->step(n, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_read_rgba8(glz_renderer* h, uint8_t* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->read_rgba8(out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_set_texture_lod(glz_renderer* h, int mode) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_texture_lod(mode, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_set_seed(glz_renderer* h, uint64_t s) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_seed(s)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_set_depth(glz_renderer* h, uint32_t d) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_depth(d, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_read_hdr(glz_renderer* h, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->read_frame(false, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_result(glz_renderer* h, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->read_frame(true, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_aov(glz_renderer* h, int which, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->post().read_aov(which, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_set_denoise(glz_renderer* h, const glz_denoise_params* p) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->post().set_denoise(p, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_set_guide_mode(glz_renderer* h, int mode, uint32_t max_bounces) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  GLZ_RET(h->r->post().set_guide_mode(mode, max_bounces, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_guide_mode(glz_renderer* h, uint32_t* max_bounces_out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  return h->r->post().guide_mode(max_bounces_out);
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_denoised(glz_renderer* h, float* rgba32f, uint8_t* rgba8) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  GLZ_RET(h->r->read_denoised(rgba32f, rgba8, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_set_despeckle(glz_renderer* h, int enabled, const glz_despeckle_params* p) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  GLZ_RET(h->r->post().set_despeckle(enabled != 0, p, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_despeckle(glz_renderer* h, glz_despeckle_params* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  return h->r->post().despeckle(out);
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_despeckled(glz_renderer* h, float* rgba32f, uint8_t* rgba8) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  GLZ_RET(h->r->read_despeckled(rgba32f, rgba8, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_motion(glz_renderer* h, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev_camera || !out) return fail(GLZ_E_ARG, "the previous camera or the output is null");
  if (prev_camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().read_motion(glz_previous_state{prev_camera, prev_transforms, n_prev_transforms, nullptr, 0, 0}, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_motion_from(glz_renderer* h, const glz_previous_state* prev, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !out) return fail(GLZ_E_ARG, "the previous state, its camera or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().read_motion(*prev, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_reproject(glz_renderer* h, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms, const float* prev_color,
                           const float* prev_aov0, const float* prev_aov1, const glz_reproject_params* params, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev_camera || !prev_color || !prev_aov0 || !prev_aov1 || !out) return fail(GLZ_E_ARG, "the previous camera, a previous frame or the output is null");
  if (prev_camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().reproject(glz_previous_state{prev_camera, prev_transforms, n_prev_transforms, nullptr, 0, 0}, prev_color, prev_aov0, prev_aov1, params, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_reproject_from(glz_renderer* h, const glz_previous_state* prev, const float* prev_color, const float* prev_aov0, const float* prev_aov1,
                                const glz_reproject_params* params, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !prev_color || !prev_aov0 || !prev_aov1 || !out) return fail(GLZ_E_ARG, "the previous state, its camera, a previous frame or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().reproject(*prev, prev_color, prev_aov0, prev_aov1, params, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_read_motion_posed(glz_renderer* h, const glz_previous_state* prev, const glz_pose* poses, uint32_t n_poses, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !out) return fail(GLZ_E_ARG, "the previous state, its camera or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().read_motion(*prev, out, e, PrevPoses{poses, n_poses, true}));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_reproject_posed(glz_renderer* h, const glz_previous_state* prev, const glz_pose* poses, uint32_t n_poses, const float* prev_color, const float* prev_aov0,
                                 const float* prev_aov1, const glz_reproject_params* params, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !prev_color || !prev_aov0 || !prev_aov1 || !out) return fail(GLZ_E_ARG, "the previous state, its camera, a previous frame or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  GLZ_RET(h->r->post().reproject(*prev, prev_color, prev_aov0, prev_aov1, params, out, e, PrevPoses{poses, n_poses, true}));
  GLZ_GUARD_END(GLZ_E_IO)
}
static PrevPoses previous_animation(const glz_animation& a) {
  PrevPoses p{a.poses, a.n_poses, true};
  p.morphs = a.morphs;
  p.n_morphs = a.n_morphs;
  return p;
}
int glz_renderer_read_motion_animated(glz_renderer* h, const glz_previous_state* prev, const glz_animation* anim, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !out) return fail(GLZ_E_ARG, "the previous state, its camera or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  if (!anim) return fail(GLZ_E_ARG, "motion: the animation is null");
  GLZ_RET(h->r->post().read_motion(*prev, out, e, previous_animation(*anim)));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_reproject_animated(glz_renderer* h, const glz_previous_state* prev, const glz_animation* anim, const float* prev_color, const float* prev_aov0,
                                    const float* prev_aov1, const glz_reproject_params* params, float* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!prev || !prev->camera || !prev_color || !prev_aov0 || !prev_aov1 || !out) return fail(GLZ_E_ARG, "the previous state, its camera, a previous frame or the output is null");
  if (prev->camera->type > GLZ_CAMERA_ORTHOGRAPHIC) return fail(GLZ_E_ARG, "unknown camera type");
  if (!anim) return fail(GLZ_E_ARG, "motion: the animation is null");
  GLZ_RET(h->r->post().reproject(*prev, prev_color, prev_aov0, prev_aov1, params, out, e, previous_animation(*anim)));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_launch_constants(glz_renderer* h, uint32_t launch, uint32_t* seed, float off[2]) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!seed || !off) return fail(GLZ_E_ARG, "output is null");
  if (!h->r->launch_constants(launch, seed, off)) return fail(GLZ_E_IO, "WorkScheduler::peek disagrees with next()");
  return GLZ_OK;
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_push_constants(glz_renderer* h, float out[32]) {
  if (!h || !out) return fail(GLZ_E_ARG, "null argument");
  h->r->push_constants(out);
  return GLZ_OK;
}
int glz_renderer_set_partition(glz_renderer* h, uint32_t rank, uint32_t world) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_partition(rank, world, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_set_devices(glz_renderer* h, const int* devices, int n) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  GLZ_RET(h->r->set_devices(devices, n, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_set_launch_mode(glz_renderer* h, int mode) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_launch_mode(mode, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_launch_mode(glz_renderer* h) { return h ? (h->r->path_mode() ? GLZ_LAUNCH_PATH : GLZ_LAUNCH_TWO_KERNELS) : 0; }
int glz_renderer_set_node_width(glz_renderer* h, int width) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_node_width(width, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_node_width(glz_renderer* h) { return h ? (h->r->wide8() ? 8 : 4) : 0; }
int glz_renderer_set_chains(glz_renderer* h, uint32_t n) { GLZ_GUARD_BEGIN GLZ_R(h); GLZ_RET(h->r->set_chains(n, e)); GLZ_GUARD_END(GLZ_E_IO) }
int glz_renderer_export_device(glz_renderer* h, int which, void* dev) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!dev) return fail(GLZ_E_ARG, "device buffer is null");
  GLZ_RET(h->r->export_device(which, dev, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
uint64_t glz_renderer_packed_pixels(glz_renderer* h, uint32_t rank, uint32_t world) {
  if (!h) return 0;
  return (uint64_t)Renderer::packed_count(h->r->width(), h->r->height(), rank, world);
}
int glz_renderer_export_packed(glz_renderer* h, int which, void* dev) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!dev) return fail(GLZ_E_ARG, "device buffer is null");
  GLZ_RET(h->r->export_packed(which, dev, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_scatter_packed(glz_renderer* h, uint32_t rank, uint32_t world, const void* packed, void* frame) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!packed || !frame) return fail(GLZ_E_ARG, "device buffer is null");
  GLZ_RET(h->r->scatter_packed(rank, world, packed, frame, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_scatter_packed_all(glz_renderer* h, uint32_t world, const void* packed, uint64_t stride_pixels, void* frame) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!packed || !frame) return fail(GLZ_E_ARG, "device buffer is null");
  GLZ_RET(h->r->scatter_packed_all(world, packed, stride_pixels, frame, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_tonemap_device(glz_renderer* h, const void* dev, uint8_t* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!dev || !out) return fail(GLZ_E_ARG, "null argument");
  GLZ_RET(h->r->tonemap_device(dev, out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}
int glz_renderer_enable_counters(glz_renderer* h, int flags) {
  if (!h) return fail(GLZ_E_ARG, "renderer is null");
  h->r->enable_counters(flags);
  return GLZ_OK;
}
int glz_renderer_get_stats(glz_renderer* h, glz_render_stats* out) {
  GLZ_GUARD_BEGIN GLZ_R(h);
  if (!out) return fail(GLZ_E_ARG, "output is null");
  GLZ_RET(h->r->get_stats(out, e));
  GLZ_GUARD_END(GLZ_E_IO)
}

int glz_renderer_device_count(glz_renderer* h) { return h ? (int)h->r->device_count() : 0; }
int glz_renderer_device_scene_info(glz_renderer* h, int i, glz_scene_info* out) {
  if (!h || !out) return fail(GLZ_E_ARG, "null argument");
  const Scene* s = h->r->device_scene(i);
  if (!s) return fail(GLZ_E_ARG, "glz_renderer_device_scene_info: no such device");
  *out = s->info;
  return GLZ_OK;
}
int glz_rccl_version(void) {
  GLZ_GUARD_BEGIN
  std::string why;
  const Rccl* nc = Rccl::get(why);
  if (!nc) return fail(GLZ_E_DEVICE, why.c_str());
  int version = 0;
  if (nc->GetVersion(&version) != ncclSuccess) return fail(GLZ_E_DEVICE, "ncclGetVersion failed");
  return version;
  GLZ_GUARD_END(GLZ_E_IO)
}

}  // extern "C"
