/* glaze_abi.h -- C ABI of libglaze_hip.so, the MI355X-native replacement for glaze's render path.
 *
 * The reference (davidepi/glaze, Rust + Vulkan-RT) has no FFI seam of its own; the seam this
 * library replaces is the public Rust API that `glaze-cli` drives (cli/src/main.rs:76-121,
 * re-exported at lib/src/lib.rs:18-22).  Every entry point below cites the reference item it
 * stands in for.  A Rust `glaze-hip-sys` binding maps
 *   status < 0  ->  io::Error / panic (the reference `expect()`s on every GPU failure),
 *   NULL handle ->  Option::None (RayTraceInstance::new, lib/src/vulkan/instance.rs:376).
 *
 * Conventions: plain pointers and sizes only; all handles opaque; every function returning
 * `int` returns 0 on success or a negative GLZ_E_* code and stores a message retrievable with
 * glz_last_error() (thread-local).  No exceptions cross the boundary.  A renderer is not
 * thread-safe (the reference takes `&mut self` on every mutator, raytracer.rs:180-326).
 */
#ifndef GLAZE_ABI_H
#define GLAZE_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLZ_OK 0
#define GLZ_E_IO (-1)          /* io::ErrorKind::NotFound / UnexpectedEof */
#define GLZ_E_INVALID_INPUT (-2) /* io::ErrorKind::InvalidInput  (bad magic / version) */
#define GLZ_E_INVALID_DATA (-3)  /* io::ErrorKind::InvalidData   (hash mismatch, corrupt xz/png) */
#define GLZ_E_ARG (-4)         /* bad argument to the C ABI itself */
#define GLZ_E_DEVICE (-5)      /* HIP failure (the reference panics here) */
#define GLZ_E_UNSUPPORTED (-6)

/* ------------------------------------------------------------------------------------------
 * Scene model PODs (host side).  Field meaning follows the reference types; layouts are this
 * ABI's own (the .glaze byte format is decoded by the library, lib/src/parser/v1.rs:631-1080).
 * ---------------------------------------------------------------------------------------- */

/* geometry/vertex.rs:6-15 -- 32 bytes, identical to the reference's #[repr(C)] Vertex. */
typedef struct glz_vertex {
  float vv[3]; /* position */
  float vn[3]; /* normal   */
  float vt[2]; /* texcoord */
} glz_vertex;

/* geometry/mesh.rs:5-16 -- indices of all meshes are concatenated in one u32 array; a mesh owns
 * [index_offset, index_offset+index_count) of it (what load_indices_to_gpu builds,
 * vulkan/scene.rs:834-850). */
typedef struct glz_mesh {
  uint16_t id;
  uint16_t material;
  uint32_t index_offset;
  uint32_t index_count;
} glz_mesh;

/* geometry/mesh.rs:29-32 -- column-major 4x4, as cgmath::Matrix4<f32>. */
typedef struct glz_transform {
  float m[16];
} glz_transform;

/* geometry/mesh.rs:23-27 */
typedef struct glz_mesh_instance {
  uint16_t mesh_id;
  uint16_t transform_id;
} glz_mesh_instance;

/* geometry/camera.rs:7-83 */
#define GLZ_CAMERA_PERSPECTIVE 0
#define GLZ_CAMERA_ORTHOGRAPHIC 1
typedef struct glz_camera {
  uint32_t type;
  float position[3];
  float target[3];
  float up[3];
  float fovx_or_scale; /* fovx (radians) for perspective, scale for orthographic */
  float near_plane;
  float far_plane;
} glz_camera;

/* materials/material.rs:17-42, ids :62-73 */
#define GLZ_MAT_FLAT 0
#define GLZ_MAT_LAMBERT 1
#define GLZ_MAT_MIRROR 2
#define GLZ_MAT_GLASS 3
#define GLZ_MAT_METAL 4
#define GLZ_MAT_FROSTED 5
#define GLZ_MAT_UBER 6
#define GLZ_NAME_MAX 256
/* materials/material.rs:290-325 */
typedef struct glz_material {
  uint8_t mtype;  /* GLZ_MAT_* */
  uint8_t metal;  /* index into materials/metal.rs:6-37 (0 = SILVER) */
  uint8_t diffuse_mul[3];
  uint8_t emissive_col[3];
  uint8_t has_emissive; /* Option<[u8;3]>::is_some() */
  uint8_t _pad[3];
  float ior;
  float roughness_mul;
  float metalness_mul;
  float anisotropy;
  uint16_t diffuse;   /* texture ids; 0 = none (white 1x1 default texture) */
  uint16_t roughness;
  uint16_t metalness;
  uint16_t normal;
  uint16_t opacity;
  uint16_t _pad2;
  char name[GLZ_NAME_MAX];
} glz_material;

/* geometry/light.rs:12-22, :146-170 */
#define GLZ_LIGHT_OMNI 0
#define GLZ_LIGHT_SUN 1
#define GLZ_LIGHT_AREA 2
#define GLZ_LIGHT_SKY 3
typedef struct glz_light {
  uint32_t ltype;
  float position[3];
  float direction[3];
  uint32_t resource_id; /* material id (AREA) or texture id (SKY) */
  float intensity;
  float yaw_deg, pitch_deg, roll_deg;
  float color[16]; /* Spectrum: 16 bins, 400..700 nm (geometry/spectrum.rs:11-24) */
  char name[GLZ_NAME_MAX];
} glz_light;

/* materials/texture.rs:94-130; only mip level 0 is used by the ray-tracing stages. */
#define GLZ_TEX_GRAY 1      /* R8_UNORM  */
#define GLZ_TEX_RGBA_SRGB 2 /* R8G8B8A8_SRGB */
#define GLZ_TEX_RGBA_NORM 3 /* R8G8B8A8_UNORM */
typedef struct glz_texture {
  uint32_t format; /* GLZ_TEX_* */
  uint32_t width, height;
  uint32_t mip_levels;   /* as stored in the file; informational */
  const uint8_t* pixels; /* level 0, tightly packed rows, 1 or 4 bytes per pixel */
  char name[GLZ_NAME_MAX];
} glz_texture;

/* parser/mod.rs:274-288 */
typedef struct glz_meta {
  float scene_centre[3];
  float scene_radius;
  float exposure;
} glz_meta;

/* In-memory scene (no reference counterpart as a type: it is what `Box<dyn ParsedScene>` hands
 * to RayTraceScene::new, vulkan/scene.rs:1414-1434).  NULL / 0 members take the reference's
 * defaults: one identity transform, one default material, one default 1x1 white texture,
 * default camera, Meta::default(). */
typedef struct glz_scene_desc {
  const glz_vertex* vertices;        uint64_t n_vertices;
  const uint32_t* indices;           uint64_t n_indices;
  const glz_mesh* meshes;            uint32_t n_meshes;
  const glz_transform* transforms;   uint32_t n_transforms;
  const glz_mesh_instance* instances;uint32_t n_instances;
  const glz_material* materials;     uint32_t n_materials;
  const glz_light* lights;           uint32_t n_lights;
  const glz_texture* textures;       uint32_t n_textures;
  const glz_camera* camera;          /* the LAST camera of the file (scene.rs:1487-1491) */
  const glz_meta* meta;
} glz_scene_desc;

/* ------------------------------------------------------------------------------------------
 * Errors
 * ---------------------------------------------------------------------------------------- */
const char* glz_last_error(void);
const char* glz_version(void);

/* ------------------------------------------------------------------------------------------
 * parse()  --  lib/src/parser/mod.rs:93-116 + ContentV1 read side (parser/v1.rs:135-175,
 * :298-362, :476-609).  Header and offset table are checked at open; chunks are decoded lazily
 * by the getters (hash mismatch -> GLZ_E_INVALID_DATA, missing chunk -> count 0).
 * Getter protocol: pass out == NULL to obtain the element count; otherwise up to `cap` elements
 * are written and the total count is returned (negative = error).
 * ---------------------------------------------------------------------------------------- */
typedef struct glz_parsed glz_parsed;
glz_parsed* glz_parse(const char* path);            /* NULL on error, see glz_last_error() */
int glz_last_status(void);                           /* status code of the last failing call on this thread */
void glz_parsed_free(glz_parsed*);
int64_t glz_parsed_vertices(glz_parsed*, glz_vertex* out, int64_t cap);           /* ParsedScene::vertices   */
int64_t glz_parsed_meshes(glz_parsed*, glz_mesh* out, int64_t cap);               /* ParsedScene::meshes     */
int64_t glz_parsed_indices(glz_parsed*, uint32_t* out, int64_t cap);              /*   (their index arrays)  */
int64_t glz_parsed_transforms(glz_parsed*, glz_transform* out, int64_t cap);      /* ParsedScene::transforms */
int64_t glz_parsed_instances(glz_parsed*, glz_mesh_instance* out, int64_t cap);   /* ParsedScene::instances  */
int64_t glz_parsed_cameras(glz_parsed*, glz_camera* out, int64_t cap);            /* ParsedScene::cameras    */
int64_t glz_parsed_materials(glz_parsed*, glz_material* out, int64_t cap);        /* ParsedScene::materials  */
int64_t glz_parsed_lights(glz_parsed*, glz_light* out, int64_t cap);              /* ParsedScene::lights     */
/* textures: `pixels` of each returned glz_texture points into memory owned by the glz_parsed. */
int64_t glz_parsed_textures(glz_parsed*, glz_texture* out, int64_t cap);          /* ParsedScene::textures   */
int glz_parsed_meta(glz_parsed*, glz_meta* out);  /* ParsedScene::meta; returns 1 if the chunk is absent (out = default) */
int glz_converted_file(const char* path);         /* parser/mod.rs:259-271: 1 if the magic matches */

/* ------------------------------------------------------------------------------------------
 * Write side.  Serializer::new(file, ParserVersion::V1).with_*(..).serialize()
 * (lib/src/parser/mod.rs:130-233; ContentV1::serialize / write_chunks, parser/v1.rs:230-295; record encoders :613-1061).
 * Every array may be empty (no chunk is written for it); `meta` NULL = Serializer without with_metadata().
 * Chunks are xz streams (LZMA2, CRC64) with an XXH64 prefix, textures are PNGs: the output is read back by glz_parse and
 * by the reference's parser alike.  glz_texture.mip_levels > 1 asks for that many levels in all, each the one before halved with the
 * Catmull-Rom filter as Texture::gen_mipmaps does (texture.rs:256-277).
 * ---------------------------------------------------------------------------------------- */
typedef struct glz_serialize_desc {
  const glz_vertex* vertices;         uint64_t n_vertices;
  const uint32_t* indices;            uint64_t n_indices;    /* index arrays of all meshes (glz_mesh.index_offset/count) */
  const glz_mesh* meshes;             uint64_t n_meshes;
  const glz_transform* transforms;    uint64_t n_transforms;
  const glz_mesh_instance* instances; uint64_t n_instances;
  const glz_camera* cameras;          uint64_t n_cameras;
  const glz_texture* textures;        uint64_t n_textures;
  const glz_material* materials;      uint64_t n_materials;
  const glz_light* lights;            uint64_t n_lights;
  const glz_meta* meta;
} glz_serialize_desc;
int glz_serialize(const char* path, const glz_serialize_desc* desc);
/* ParsedScene::update (parser/v1.rs:364-422): rewrites the parsed file in place with the given chunks replaced and
 * re-reads it.  A count of -1 (or meta == NULL) keeps that chunk exactly as stored; geometry is always kept.  Pointers
 * obtained earlier from this handle's getters are invalidated. */
int glz_parsed_update(glz_parsed*, const glz_camera* cameras, int64_t n_cameras, const glz_material* materials, int64_t n_materials,
                      const glz_light* lights, int64_t n_lights, const glz_texture* textures, int64_t n_textures, const glz_meta* meta);

/* image.save(path) of the CLI (cli/src/main.rs:121): RGBA8 rows top-down -> PNG (RGBA) or baseline JPEG (alpha dropped,
 * quality 75) chosen by the extension (.png / .jpg / .jpeg). */
int glz_save_image(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);
/* glaze-converter for Wavefront OBJ input (converter/src/main.rs:116-637 without assimp): OBJ + MTL + PNG / baseline-JPEG
 * textures -> .glaze V1 with the reference converter's layout (default material/texture first, "DefaultMaterial" second,
 * de-duplicated flipped-v vertices, one identity transform, AREA lights for emissive materials, default camera, Meta
 * from the bounds).  gen_mipmaps != 0 stores the full mip chain (--gen-mipmaps).  counts (may be NULL) receives
 * {vertices, triangles, meshes, materials, textures, lights}. */
int glz_convert_obj(const char* input_obj, const char* output_glaze, int gen_mipmaps, uint64_t counts[6]);

/* ------------------------------------------------------------------------------------------
 * RayTraceInstance::new() -> Option<Self>   (lib/src/vulkan/instance.rs:376-427)
 * hip_device = -1 picks the first gfx950 device (LOCAL_RANK-agnostic; pass the ordinal for
 * one-process-per-GPU jobs).  NULL <=> None: no usable device or the HIP code object is missing.
 * ---------------------------------------------------------------------------------------- */
typedef struct glz_instance glz_instance;
glz_instance* glz_instance_create(int hip_device);
void glz_instance_destroy(glz_instance*);
int glz_instance_device(const glz_instance*);
/* stream all of this instance's kernels run on (a hipStream_t), for event timing by the caller */
void* glz_instance_stream(const glz_instance*);
/* [extension] acceleration-structure builder for scenes created afterwards (the reference leaves the choice to the
 * Vulkan driver, acceleration.rs:253-257 asks for PREFER_FAST_TRACE).  Hits do not depend on it.
 *   GLZ_BVH_SAH      (default, = GLZ_BVH_AUTO) top-down binned SAH on the GPU, level by level: 7 ms for 262 k
 *                    triangles, 14 ms for 1.8 M, 34 ms for 7 M, 86 ms for 21 M; SAH cost -11 % and 5-13 % more samples
 *                    per second than the LBVH
 *   GLZ_BVH_LBVH     Karras 2012 on the GPU: fastest build (3 ms for 262 k triangles, 33 ms for 21 M)
 *   GLZ_BVH_PLOC     parallel locally-ordered clustering on the GPU (Meister & Bittner 2018): the LBVH's quality here
 *   GLZ_BVH_SAH_HOST the SAH builder's reference implementation on the host cores: the same tree node for node, 3-24 x
 *                    slower (tests compare the two)
 * Size limit, whichever builder: the kernels address the hierarchy with 32-bit byte offsets, so scene creation (and every later
 * rebuild) fails with GLZ_E_INVALID_DATA when a table would reach 2^32 bytes -- 2^26 4-wide nodes or leaf records (64 bytes each), 2^25
 * 8-wide nodes (128), 2^32 / 192 instance records, or a traversal-stack spill area (lanes of the largest persistent grid x words a
 * lane spills, which grows with the hierarchy's depth) of 2^30 words.  A 21 M triangle scene is at a tenth of the nearest of these. */
#define GLZ_BVH_LBVH 0
#define GLZ_BVH_PLOC 1
#define GLZ_BVH_SAH 2
#define GLZ_BVH_AUTO 3
#define GLZ_BVH_SAH_HOST 4
int glz_instance_set_bvh_builder(glz_instance*, int builder);
/* [extension] shape of the acceleration structure of scenes created afterwards.  The reference keeps one BLAS per mesh and a TLAS
 * over the instances (acceleration.rs:319-345).  GLZ_AS_AUTO (default): two levels when the instances hold more than four
 * times the triangles of the meshes they share, else ONE hierarchy over world-space triangles (fastest to trace, memory
 * grows with instances x triangles); GLZ_AS_FLAT / GLZ_AS_TWO_LEVEL force either.  Hits are bit-identical both ways: inside an
 * instance only the box tests run in object space, the triangle test stays in world space. */
#define GLZ_AS_AUTO 0
#define GLZ_AS_FLAT 1
#define GLZ_AS_TWO_LEVEL 2
int glz_instance_set_as_levels(glz_instance*, int mode);

/* ------------------------------------------------------------------------------------------
 * RayTraceScene::new(instance, parsed)   (lib/src/vulkan/scene.rs:1414-1556)
 * Uploads geometry, runs the derivative kernel (scene.rs:2113-2188), builds the LBVH that
 * replaces SceneASBuilder (vulkan/acceleration.rs:89-494), builds RTInstance/RTMaterial/RTLight
 * arrays (scene.rs:1784-1927) and the sky sampling tables (scene.rs:2191-2313).
 * glz_scene_create consumes `parsed` (it is freed, as the Box is moved in the reference).
 * ---------------------------------------------------------------------------------------- */
typedef struct glz_scene glz_scene;
glz_scene* glz_scene_create(glz_instance*, glz_parsed* parsed);
glz_scene* glz_scene_create_from_desc(glz_instance*, const glz_scene_desc*);
void glz_scene_destroy(glz_scene*);

typedef struct glz_scene_info {
  uint64_t n_vertices, n_triangles;          /* object-space triangles over all meshes */
  uint64_t n_world_triangles;                /* after instancing (BVH primitives)       */
  uint32_t n_instances, n_materials, n_lights /* lights_no, scene.rs:1549 */, n_rt_lights, n_textures;
  uint32_t bvh_nodes, bvh_depth;
  float bvh_sah_cost;                        /* of the last BUILD: a refit (glz_renderer_update_vertices) keeps the topology and leaves this figure, bvh_depth, bvh_nodes* and as_bytes alone */
  float build_ms;                            /* hierarchy build time on the device (whichever builder); after update_vertices the update's stream time */
  float bounds_min[3], bounds_max[3];
  float bvh_grid_lo[3], bvh_grid_cell[3];    /* quantisation grid of the BVH node boxes: world = lo + q * cell */
  uint32_t as_levels;                        /* 1 = one hierarchy over all instanced triangles, 2 = TLAS over per-mesh BLAS */
  uint32_t n_as_triangles;                   /* triangle records the structure holds (= n_world_triangles when flattened) */
  uint64_t as_bytes;                         /* device bytes of nodes + triangle / leaf records + shading records + instance records */
  uint32_t bvh_nodes8, _reserved;            /* 8-wide nodes of the same hierarchy (the tracer of small tile shares; flattened builds), 0 = none */
} glz_scene_info;
int glz_scene_get_info(const glz_scene*, glz_scene_info* out);
int glz_scene_camera(const glz_scene*, glz_camera* out);

/* ------------------------------------------------------------------------------------------
 * RayTraceRenderer   (lib/src/vulkan/raytracer.rs:109-687)
 * ---------------------------------------------------------------------------------------- */
typedef struct glz_renderer glz_renderer;
#define GLZ_DIRECT 0      /* Integrator::DIRECT      raytracer.rs:36-52 */
#define GLZ_PATH_TRACE 1  /* Integrator::PATH_TRACE */

/* RayTraceRenderer::new(instance, Some(scene), w, h)  raytracer.rs:164-177; the renderer owns
 * the scene from here on (raytracer.rs:109-111): do not destroy it yourself. */
glz_renderer* glz_renderer_create(glz_instance*, glz_scene* scene, uint32_t width, uint32_t height);
void glz_renderer_destroy(glz_renderer*);
int glz_renderer_set_integrator(glz_renderer*, int integrator);          /* raytracer.rs:196-231 */
int glz_renderer_set_exposure(glz_renderer*, float exposure);            /* raytracer.rs:180-194 */
int glz_renderer_update_camera(glz_renderer*, const glz_camera*);        /* raytracer.rs:300-309 */
int glz_renderer_change_resolution(glz_renderer*, uint32_t w, uint32_t h);/* raytracer.rs:250-298 */
int glz_renderer_change_scene(glz_renderer*, glz_scene* scene);          /* raytracer.rs:233-248 */
/* raytracer.rs:311-326 (&[Material], &[Light], &[Texture]): rebuilds RTMaterial / RTLight / sky tables; restarts
 * accumulation.  The material count must not change.  `textures` NULL keeps the scene's texture array; otherwise it
 * replaces it (level 0 is uploaded; the reference needs the raw textures for the sky distributions, scene.rs:1598-1615). */
int glz_renderer_update_materials_and_lights(glz_renderer*, const glz_material* mats, uint32_t n_mats,
                                             const glz_light* lights, uint32_t n_lights,
                                             const glz_texture* textures, uint32_t n_textures);
/* Moves the instances: `transforms` replaces the scene's object -> world matrices (as many as the scene has: instances index them
 * by a 16-bit id, and the count cannot change).  Waits for the renderer to go idle; restarts accumulation (a later step(k) / draw
 * equals a fresh renderer's on a scene created with these transforms, same seed); reaches every device of set_devices.  The
 * update acts on the SCENE object, so other renderers that share the scene see it too, as with materials.  The structure is
 * rebuilt with the builder and shape the scene was created with: a flattened scene is built again in full; a two-level scene keeps
 * its meshes' hierarchies and rebuilds only the top level.  Non-finite or singular transforms are taken as creation takes them.
 * GLZ_E_ARG (nothing changes): null transforms, a different count. */
int glz_renderer_update_transforms(glz_renderer*, const glz_transform* transforms, uint32_t n_transforms);
/* Build-defined (the reference has nothing like it): deforming meshes.  Replaces vertices [first_vertex, first_vertex + n_vertices) of
 * the scene's vertex buffer: positions, normals, texture coordinates.  Indices, meshes, instances, transforms, materials, lights and
 * textures stay.  Waits for the renderer to go idle; restarts accumulation; reaches every device of set_devices; acts on the SCENE
 * object, so every renderer sharing the scene sees the change (as with update_transforms).  Afterwards hits and renders equal, bit for
 * bit, those of a scene created with the new vertices, in both modes:
 *   GLZ_GEOMETRY_REFIT    the hierarchy keeps its topology; leaf records, boxes and the quantisation grid are refitted on the device (a
 *                         two-level scene refits the meshes whose indices reach into the range and rebuilds its top level);
 *   GLZ_GEOMETRY_REBUILD  the builder runs again, with the options and the shape the scene was created with.
 * A refitted tree traces the slower the further the mesh has moved from the shape it was built for: glz_geometry_update_info gives the
 * figure to decide on a rebuild by (the library never rebuilds on its own).  After a refit glz_scene_info's bounds_* and bvh_grid_* are
 * the new ones and build_ms is the update's stream time; bvh_sah_cost, bvh_depth, bvh_nodes* and as_bytes are those of the last build.
 * GLZ_E_ARG (the scene is untouched): null vertices, n_vertices == 0, a range past the vertex count, an unknown mode.  (Creation checks
 * index ranges and references, never positions: there is no position it would refuse, and none is refused here.) */
#define GLZ_GEOMETRY_REFIT   0   /* keep the topology, refit boxes and records (default) */
#define GLZ_GEOMETRY_REBUILD 1   /* run the builder again, with the options and shape the scene was created with */
int glz_renderer_update_vertices(glz_renderer*, const glz_vertex* vertices, uint32_t first_vertex, uint32_t n_vertices, int mode);
typedef struct glz_geometry_update_info {
  uint32_t mode;            /* what the last update_vertices did */
  uint32_t meshes_touched;  /* two-level scenes: meshes whose hierarchy was refitted / rebuilt; flattened: 1 */
  float    update_ms;       /* device-event time on the stream: upload to last kernel */
  float    box_area;        /* sum of the surface areas of all child boxes of the 4-wide nodes (two levels: of the meshes' nodes) after the update (float, reported only: the sum's order is not fixed) */
  float    box_area_built;  /* the same sum for the structure as the builder left it (taken on the first refit after a build, before the new vertices go in; after a rebuild, of the new structure) */
} glz_geometry_update_info;
int glz_renderer_geometry_update_info(glz_renderer*, glz_geometry_update_info* out);   /* GLZ_E_ARG before any update */
/* Build-defined: skinned meshes -- linear-blend skinning on the device, so that a posed character costs a few matrices over the bus a frame
 * instead of its vertices.
 *
 *   THE SKINNING RULE (glz_renderer_pose_skins, glz_host_skin; one definition, glaze_amd/csrc/skin.h, compiled for host and device; the
 *   tests hold both sides to this text bit for bit).  float32 throughout, only + and x, no contraction into fused multiply-adds, the
 *   operations in exactly this order.  A vertex has bind position p, bind normal n, texture coordinate t, joints j0..j3 and weights w0..w3;
 *   the bone matrices B[k] are glz_transform, column-major (element [r][c] is m[4 * c + r]); only the upper 3 x 4 is read, the fourth row
 *   is ignored.  For row r in 0..2 and column c in 0..3:
 *     M[r][c] = ((w0 * B[j0][r][c] + w1 * B[j1][r][c]) + w2 * B[j2][r][c]) + w3 * B[j3][r][c]
 *     p'[r]   = ((M[r][0] * p.x + M[r][1] * p.y) + M[r][2] * p.z) + M[r][3]
 *     n'[r]   =  (M[r][0] * n.x + M[r][1] * n.y) + M[r][2] * n.z
 *     t'      = t
 *   No term is skipped for a zero weight (0 x inf is NaN here too).  Weights are used as given and are not normalised.  The normal goes
 *   through M's 3 x 3 and is not renormalised (shading normalises the normal it interpolates): that is exact only for rigid bones.  Bones
 *   act in the mesh's OBJECT space, where the vertex buffer lives; the caller supplies joint_now x inverse_bind per bone -- or gives the
 *   skin a skeleton and plays clips on it (glz_renderer_play, THE CLIP RULE), and the device makes these matrices itself.
 *
 *   THE DUAL-QUATERNION RULE (a skin set to GLZ_SKIN_DUAL_QUATERNION; glz_host_skin_dq, glz_host_bone_dual_quats; one definition,
 *   glaze_amd/csrc/skin.h and skin_host.cpp, the per-vertex part compiled for host and device; the tests hold both sides to this text bit
 *   for bit).  The caller's side does not change: a pose still carries glz_transform matrices, joint_now x inverse_bind in object space.
 *   Linear blending of two rigid bones is not rigid (a half-turn twist at weights 1/2 : 1/2 collapses to a line); the normalised blend of
 *   their unit dual quaternions is, so positions keep their distance to the joint and the normal is exact, for rigid bones.
 *
 *   BONE CONVERSION, on the host only, once per bone per pose, for the device upload and the host reference alike: float64 throughout,
 *   the operations in exactly this order, rounded to float32 at the end.  mRC is element m[4 * C + R]; only the upper 3 x 4 is read.
 *     tr = (m00 + m11) + m22
 *     if tr > 0:                        s = 2 * sqrt(tr + 1);                   w = s / 4;           x = (m21 - m12) / s;  y = (m02 - m20) / s;  z = (m10 - m01) / s
 *     else if m00 > m11 and m00 > m22:  s = 2 * sqrt(((1 + m00) - m11) - m22);  w = (m21 - m12) / s;  x = s / 4;           y = (m01 + m10) / s;  z = (m02 + m20) / s
 *     else if m11 > m22:                s = 2 * sqrt(((1 + m11) - m00) - m22);  w = (m02 - m20) / s;  x = (m01 + m10) / s;  y = s / 4;           z = (m12 + m21) / s
 *     else:                             s = 2 * sqrt(((1 + m22) - m00) - m11);  w = (m10 - m01) / s;  x = (m02 + m20) / s;  y = (m12 + m21) / s;  z = s / 4
 *     len = sqrt(((x * x + y * y) + z * z) + w * w);   x = x / len;  y = y / len;  z = z / len;  w = w / len
 *     (tx, ty, tz) = (m03, m13, m23)
 *     dx = 0.5 * ((tx * w + ty * z) - tz * y)
 *     dy = 0.5 * ((ty * w + tz * x) - tx * z)
 *     dz = 0.5 * ((tz * w + tx * y) - ty * x)
 *     dw = -(0.5 * ((tx * x + ty * y) + tz * z))
 *   A comparison with a NaN is false (such a matrix takes the last branch).  A uniform scale drops out in the division by len; the 3 x 3
 *   is otherwise used as given: a matrix that is no rotation gives this text's image of it and no more.  Nothing is checked.  A bone as
 *   the kernels read it is two float4, q = (x, y, z, w) then d = (dx, dy, dz, dw): 32 bytes against the skinning rule's 48.
 *
 *   PER VERTEX: float32 throughout, + - x, one square root and one division (both correctly rounded), no contraction into fused
 *   multiply-adds, the operations in exactly this order.  q_k, d_k are the two parts of bone j_k, k in 0..3.
 *     1. signs     c0 = w0;  for k in 1..3:  dot_k = ((q0.x * qk.x + q0.y * qk.y) + q0.z * qk.z) + q0.w * qk.w;  c_k = -w_k if dot_k < 0 else w_k
 *     2. blend     R.e = ((c0 * q0.e + c1 * q1.e) + c2 * q2.e) + c3 * q3.e   and   D.e = the same sum over d_k,   e in x, y, z, w
 *     3. normalise nn = ((R.x * R.x + R.y * R.y) + R.z * R.z) + R.w * R.w;   inv = 1 / sqrt(nn);   r = R * inv;   d = D * inv
 *     4. translate T.x = 2 * (((r.w * d.x - d.w * r.x) + r.y * d.z) - r.z * d.y)      (T.y, T.z: x -> y -> z -> x in every subscript but w)
 *     5. rotate    a.x = (r.y * v.z - r.z * v.y) + r.w * v.x;   b.x = r.y * a.z - r.z * a.y;   rot(v).x = v.x + 2 * b.x     (y, z: cyclic)
 *     6. result    p' = rot(p) + T;   n' = rot(n);   t' = t
 *   The pivot of the sign step is j0 whatever its weight; a dot of -0, +0 or NaN keeps the weight's sign.  No term is skipped for a zero
 *   weight.  Weights are used as given and are NOT normalised (step 3 removes their common factor).  nn == 0 is NOT special-cased: 1 /
 *   sqrt(0) is infinite and the vertex comes out non-finite, on both sides alike.  The normal is not renormalised: r is a unit quaternion
 *   up to rounding, so |n'| = |n| up to rounding, and a skin in this mode needs no normal set for what its bones do.
 *
 * glz_renderer_add_skin: a skin over the vertices [first_vertex, first_vertex + n_vertices).  Its bind pose is what the scene's vertices
 * hold in that range at the moment of the call (copied on the device into a buffer the skin owns); joints (4 per vertex) and weights (4
 * per vertex) are uploaded once.  Returns the skin's id (>= 0).  Skins belong to the SCENE object, as the vertices do: every renderer
 * sharing the scene sees them, and every device of set_devices gets them.  GLZ_E_ARG (nothing changes): a null pointer, n_vertices == 0, a
 * range past the vertex count, n_bones == 0 (or above 65536), a joint >= n_bones, a range that overlaps an existing skin.
 * glz_renderer_remove_skin frees a skin; the vertices stay as they are.  GLZ_E_ARG: no such skin. */
typedef struct glz_skin {
  uint32_t        first_vertex;
  uint32_t        n_vertices;
  const uint16_t* joints;    /* 4 * n_vertices, each < n_bones */
  const float*    weights;   /* 4 * n_vertices */
  uint32_t        n_bones;
} glz_skin;
int glz_renderer_add_skin(glz_renderer*, const glz_skin*);
int glz_renderer_remove_skin(glz_renderer*, int skin);
/* A skin's blend mode: which of the two rules above poses it.  A new skin is GLZ_SKIN_LINEAR, which is exactly what a skin was before the
 * mode existed.  Setting the mode writes no vertex and restarts nothing: the library keeps no bones between calls, so the next
 * glz_renderer_pose_skins / glz_renderer_animate, and the previous-pose passes of read_motion_posed / reproject_posed and their _animated
 * forms, convert their bones for the mode and run its kernel (k_skin_dq; k_morph_skin_dq where the skin's morph is named too).  Every
 * device of set_devices follows, and a device attached later gets the mode with the skin.  glz_renderer_skin_blend returns the mode.
 * GLZ_E_ARG (nothing changes): an unknown skin, an unknown mode. */
#define GLZ_SKIN_LINEAR          0   /* THE SKINNING RULE (default) */
#define GLZ_SKIN_DUAL_QUATERNION 1   /* THE DUAL-QUATERNION RULE */
int glz_renderer_set_skin_blend(glz_renderer*, int skin, int blend);
int glz_renderer_skin_blend(glz_renderer*, int skin);
/* Poses one or more skins and updates the structure ONCE: the bones of every named skin go up, the rule runs per skin from its bind pose
 * into the scene's vertices, then the derivatives and the structure follow as in glz_renderer_update_vertices (`mode`: GLZ_GEOMETRY_*),
 * over the span from the lowest to the highest posed vertex.  Everything update_vertices promises holds: idle first, accumulation
 * restarts, every device of set_devices follows, glz_renderer_geometry_update_info describes it (update_ms: bone upload to last kernel),
 * and afterwards hits and renders equal, bit for bit, those of a scene created with the vertices glz_host_skin gives.  A later
 * update_vertices over a skinned range is allowed: it overwrites the current vertices, the bind pose stays, the next pose overwrites them
 * again.  GLZ_E_ARG (the scene is untouched): a null pointer or n_poses == 0, an unknown skin, the same skin named twice, null bones,
 * n_bones different from the skin's, an unknown mode. */
typedef struct glz_pose {
  int                  skin;
  const glz_transform* bones;   /* n_bones matrices: joint_now x inverse_bind, object space */
  uint32_t             n_bones; /* the skin's */
} glz_pose;
int glz_renderer_pose_skins(glz_renderer*, const glz_pose* poses, uint32_t n_poses, int mode);
/* The scene's current vertices [first_vertex, first_vertex + n_vertices) as the device holds them (idle first).  GLZ_E_ARG: null output,
 * n_vertices == 0, a range past the vertex count. */
int glz_renderer_read_vertices(glz_renderer*, uint32_t first_vertex, uint32_t n_vertices, glz_vertex* out);
/* Build-defined: morph targets (blend shapes) -- applied on the device, ahead of the skin, so that a morphed character costs a few weights
 * over the bus a frame instead of its vertices.
 *
 *   THE MORPH RULE (glz_renderer_animate, glz_host_morph; one definition, glaze_amd/csrc/morph.h, compiled for host and device; the tests
 *   hold both sides to this text bit for bit).  A morph covers the vertices [first_vertex, first_vertex + n_vertices) and has n_targets
 *   targets, 1 .. 65536.  Target t is a list of entries (v, dp[3], dn[3]): v is a vertex index relative to first_vertex, STRICTLY
 *   ASCENDING within the target, so a target touches a vertex at most once.  A target given without an index list (vertices == NULL) is
 *   dense: entry e is vertex e, and there are n_vertices of them.  d_normal is required; a caller without normal deltas passes zeros.
 *   For a vertex with base position p, base normal n and texture coordinate t, let t1 < t2 < ... < tk be the targets that have an entry
 *   for it, with weights w[ti] and deltas dp_i, dn_i.  Per component, in float32, with no contraction into fused multiply-adds, and in
 *   exactly this order:
 *     p' = ((…((p + w[t1] * dp_1) + w[t2] * dp_2) …) + w[tk] * dp_k)
 *     n' = ((…((n + w[t1] * dn_1) + w[t2] * dn_2) …) + w[tk] * dn_k)
 *     t' = t
 *   No term is skipped for a zero weight (0 x inf is NaN here too, and -0 + 0 x d is +0).  Weights are used as given; the normal is not
 *   renormalised.  A vertex no target touches comes out with the bits it went in with.
 *   COMPOSITION WITH A SKIN: the morphed vertex is the BIND vertex THE SKINNING RULE then sees; the result equals
 *   glz_host_skin(glz_host_morph(bind, ...), ...) bit for bit -- glz_host_skin_dq(glz_host_morph(bind, ...), ...) for a skin in
 *   GLZ_SKIN_DUAL_QUATERNION mode, whose fused kernel applies THE DUAL-QUATERNION RULE instead.
 *
 * glz_renderer_add_morph returns the morph's id (>= 0).  The targets are transposed once, on the host, into the layout the kernels read
 * and uploaded; the caller's arrays are not kept.  A FREE-STANDING morph (skin == -1) owns a copy of its base, made on the device from
 * what the scene's vertices hold in the range at the moment of the call; its range may overlap no other morph and no skin.  An ATTACHED
 * morph (skin >= 0) has exactly its skin's range, its base IS the skin's bind pose (no copy), and a skin carries at most one;
 * glz_renderer_remove_skin of a skin that still carries a morph is refused (GLZ_E_ARG).  Morphs belong to the SCENE object, as skins do:
 * ids count up and are never reused, and every device of set_devices gets them.  GLZ_E_ARG (nothing changes): a null pointer,
 * n_vertices == 0, a range past the vertex count, n_targets out of 1 .. 65536, an entry index >= n_vertices, indices not strictly
 * ascending, a dense target whose n != n_vertices, null deltas where n > 0 (a target with n == 0 is allowed), an overlap (free-standing),
 * an unknown skin, a skin that already has a morph, or a range that is not the skin's (attached).
 * glz_renderer_remove_morph frees a morph; the vertices stay as they are.  GLZ_E_ARG: no such morph. */
typedef struct glz_morph_target {
  const uint32_t* vertices;     /* n indices relative to the morph's first vertex, strictly ascending; NULL: dense */
  const float*    d_position;   /* 3 * n */
  const float*    d_normal;     /* 3 * n */
  uint32_t        n;
} glz_morph_target;
typedef struct glz_morph {
  uint32_t                first_vertex, n_vertices;
  const glz_morph_target* targets;
  uint32_t                n_targets;
  int                     skin;   /* -1: free-standing */
} glz_morph;
int glz_renderer_add_morph(glz_renderer*, const glz_morph*);
int glz_renderer_remove_morph(glz_renderer*, int morph);
/* Morphs and poses in one call, and the structure updated ONCE, over the span from the lowest to the highest vertex written.  A named
 * free-standing morph is blended from its base into the scene's vertices; a named skin whose morph is not named is posed as
 * glz_renderer_pose_skins poses it (from its unmorphed bind pose); a named skin whose morph is also named goes through the fused kernel:
 * THE MORPH RULE, then THE SKINNING RULE, the vertex never in memory in between.  With n_morphs == 0 it is glz_renderer_pose_skins, and
 * everything that promises holds: idle first, accumulation restarts, every device follows, glz_renderer_geometry_update_info describes it,
 * hits and renders equal those of a scene created with the vertices the host references give.  The library keeps no weights and no bones
 * between calls: every call starts from the bases.  GLZ_E_ARG (the scene is untouched): a null animation, or nothing named; an unknown
 * morph, or a morph named twice; null weights; n_targets not the morph's; an attached morph named without its skin's pose; the pose
 * checks of glz_renderer_pose_skins; an unknown mode.  glz_renderer_pose_skins itself knows nothing of morphs. */
typedef struct glz_morph_weights {
  int          morph;
  const float* weights;     /* n_targets */
  uint32_t     n_targets;   /* the morph's */
} glz_morph_weights;
typedef struct glz_animation {
  const glz_morph_weights* morphs;
  uint32_t                 n_morphs;
  const glz_pose*          poses;
  uint32_t                 n_poses;
} glz_animation;
int glz_renderer_animate(glz_renderer*, const glz_animation*, int mode);
/* Build-defined: skeletons and clips -- the bone tables (and morph weight tables) of playing characters made ON THE DEVICE from keyframes
 * uploaded once, so that a frame of a playing crowd sends one small record per character and no bone crosses the bus.
 *
 *   THE CLIP RULE (glz_renderer_play, glz_host_clip_bones; one definition, glaze_amd/csrc/clip.h, compiled for host and device; the tests
 *   hold both sides to this text bit for bit).  float32 throughout, + - x, one 1 / sqrt per bone (both operations correctly rounded), no
 *   contraction into fused multiply-adds, the operations in exactly this order.  A skeleton has n_bones bones; parents[b] is -1 for a root,
 *   else below b.  A clip has n_keys keys at times[k], strictly ascending; key k holds, per bone, a translation (3), a rotation (x, y, z,
 *   w; used as given, not normalised) and a scale (3), and optionally one weight per morph target.  Matrices are 3 x 4, [r][c].
 *     1. key choice (on the host, in float32, for the reference and the device alike; the kernel receives the triple, never t):
 *          t <= times[0]:     (k0, k1, u) = (0, 0, 0)
 *          t >= times[last]:  (k0, k1, u) = (last, last, 0)
 *          else:              k0 = the largest k with times[k] <= t;  k1 = k0 + 1;  u = (t - times[k0]) / (times[k1] - times[k0])
 *     2. lerp(a, b) = a + u * (b - a)  per component, for translation, scale and morph weights.  No term is skipped: with k0 == k1 a finite
 *        value comes back as it is, an infinity becomes NaN.
 *     3. rotation, a normalised lerp with a hemisphere step: a, b the rotations of keys k0, k1
 *          dot = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;   b enters negated if dot < 0 (a dot of -0, +0 or NaN keeps it)
 *          Q = lerp(a, +-b);   nn = ((Q.x * Q.x + Q.y * Q.y) + Q.z * Q.z) + Q.w * Q.w;   inv = 1 / sqrt(nn);   q = Q * inv
 *        nn == 0 is NOT special-cased.
 *     4. local matrix from (t, q, s), with xx = q.x * q.x, xy = q.x * q.y, ... wz = q.w * q.z:
 *          R00 = 1 - 2 * (yy + zz)   R01 = 2 * (xy - wz)       R02 = 2 * (xz + wy)
 *          R10 = 2 * (xy + wz)       R11 = 1 - 2 * (xx + zz)   R12 = 2 * (yz - wx)
 *          R20 = 2 * (xz - wy)       R21 = 2 * (yz + wx)       R22 = 1 - 2 * (xx + yy)
 *          L[r][c] = R[r][c] * s[c]  (c in 0..2; without a scale track s = 1 and the product is still formed),   L[r][3] = t[r]
 *     5. affine product C = A o B:
 *          C[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]                      c in 0..2
 *          C[r][3] = ((A[r][0] * B[0][3] + A[r][1] * B[1][3]) + A[r][2] * B[2][3]) + A[r][3]
 *     6. hierarchy:  W[b] = root o L[b] for a root, else W[parents[b]] o L[b] -- the product always runs down the chain and is never
 *        regrouped, so the order bones are evaluated in does not reach the bits.   The bone is B[b] = W[b] o inverse_bind[b].
 *     7. table: for a linear skin the three rows of B[b] (what glz_renderer_pose_skins uploads for that matrix); for a skin in
 *        GLZ_SKIN_DUAL_QUATERNION mode the BONE CONVERSION above applied to B[b] -- float64, in that text's order, rounded to float32 at
 *        the end -- which the device computes with the same definition the host does.
 *   CONSEQUENCE: glz_renderer_play(clip, t) leaves the vertices glz_renderer_pose_skins leaves when given glz_host_clip_bones(..., t), bit
 *   for bit, in either blend mode; with a weight track, those glz_renderer_animate leaves when given those bones and the lerped weights.
 *   Interpolation is nlerp, not slerp: keys are expected to be dense enough.  Keys are uniform across bones, as in a baked clip.
 *
 * glz_renderer_add_skeleton returns the skeleton's id (>= 0; ids count up and are never reused).  Skeletons and clips belong to the SCENE
 * object, as skins do, and every device of set_devices gets them under the same ids.  The level table (bones grouped by depth) is made
 * on the host; it, parents, inverse_bind and root are uploaded once, and the skeleton's world and bone tables are allocated on the
 * device (the bone table for the larger blend mode, so glz_renderer_set_skin_blend reallocates nothing).  Only the upper 3 x 4 of
 * inverse_bind and root is read; root is what roots are multiplied under, so the skin's object space may differ from the skeleton's.
 * GLZ_E_ARG (nothing changes): a null pointer, an unknown skin, n_bones not the skin's, a skin that already has a skeleton, a parent
 * that is neither -1 nor below its bone.  glz_renderer_remove_skeleton frees it AND its clips; glz_renderer_remove_skin of a skin that
 * still has a skeleton is refused (GLZ_E_ARG), and so is glz_renderer_remove_morph of a morph that a clip's weight track still drives.
 * glz_renderer_add_clip returns the clip's id (>= 0, counting up, never reused); the clip is uploaded once.  scales == NULL: every scale
 * is 1.  morph_weights (n_keys x n_targets) is allowed only when the skeleton's skin carries an attached morph with n_targets targets;
 * NULL (with n_targets 0): the clip does not drive the morph.  GLZ_E_ARG (nothing changes): a null pointer, an unknown skeleton,
 * n_keys == 0, times not finite or not strictly ascending, null translations or rotations, a weight track without such a morph or with
 * another target count.  glz_renderer_remove_clip frees a clip. */
typedef struct glz_skeleton {
  int                  skin;           /* ignored by glz_host_clip_bones */
  uint32_t             n_bones;        /* the skin's */
  const int32_t*       parents;        /* n_bones: -1 a root, else < the bone's own index */
  const glz_transform* inverse_bind;   /* n_bones */
  glz_transform        root;
} glz_skeleton;
typedef struct glz_clip {
  int          skeleton;        /* ignored by glz_host_clip_bones */
  uint32_t     n_keys;          /* >= 1 */
  const float* times;           /* n_keys, finite, strictly ascending */
  const float* translations;    /* n_keys x n_bones x 3 */
  const float* rotations;       /* n_keys x n_bones x 4: (x, y, z, w) */
  const float* scales;          /* n_keys x n_bones x 3, or NULL */
  const float* morph_weights;   /* n_keys x n_targets, or NULL */
  uint32_t     n_targets;
} glz_clip;
int glz_renderer_add_skeleton(glz_renderer*, const glz_skeleton*);
int glz_renderer_remove_skeleton(glz_renderer*, int skeleton);
int glz_renderer_add_clip(glz_renderer*, const glz_clip*);
int glz_renderer_remove_clip(glz_renderer*, int clip);
/* Plays clips and updates the structure ONCE.  One launch of k_clip_bones makes the bone table of every named clip's skeleton, in its
 * skin's blend layout, and the weight table of every clip that has a weight track; then each skin is deformed from its bind pose by the
 * kernel glz_renderer_animate would use -- the fused morph kernel where the clip has a weight track -- reading those tables where they
 * are.  The only upload is one small table for the whole call: per play the clip, (k0, k1, u) and the blend mode.  Everything
 * glz_renderer_animate promises holds: idle first, accumulation restarts, the structure is updated once (`mode`: GLZ_GEOMETRY_*) over the
 * span from the lowest to the highest vertex written, every device of set_devices follows, normal sets whose reach overlaps the span
 * run afterwards, glz_renderer_geometry_update_info describes it.  Nothing is kept between calls: every call starts from the bind pose.
 * glz_renderer_pose_skins and glz_renderer_animate keep working on a skin that has a skeleton.  GLZ_E_ARG (the scene is untouched): a
 * null pointer or n_plays == 0, an unknown clip, two plays whose clips belong to the same skeleton, a non-finite time, an unknown mode. */
typedef struct glz_play {
  int   clip;
  float time;
} glz_play;
int glz_renderer_play(glz_renderer*, const glz_play* plays, uint32_t n_plays, int mode);
/* Build-defined: shading normals recomputed on the device from the positions it holds -- after a pose, a morph or new positions from the
 * caller -- so that a deformed surface is shaded with the normals of the shape it has now.  Opt-in per vertex range: without a normal set
 * nothing changes.
 *
 *   THE NORMAL RULE (glz_renderer_add_normals, glz_host_vertex_normals; one definition, glaze_amd/csrc/normals.h, compiled for host and
 *   device; the tests hold both sides to this text bit for bit).  float32 throughout, no contraction into fused multiply-adds; only
 *   + - x, one sqrtf and one 1.0f / x, both correctly rounded.  A NORMAL SET covers the vertices [first_vertex, first_vertex + n_vertices).
 *   TRIANGLES: mesh m of the scene's mesh array, in array order, has the triangles k < index_count / 3 with corners
 *   indices[index_offset + 3k + c]; triangles are ordered by (m, k).  Mesh index ranges need not be disjoint: two meshes over the same
 *   indices contribute their triangles twice, and nothing is done about it.  The set's FACES are the triangles with at least one corner
 *   in the range, in that order.
 *   FACE VECTOR of a face with corner positions p0, p1, p2, read from the current vertex buffer (corners outside the range are read and
 *   never written):
 *     a = p1 - p0, b = p2 - p0 (per component)
 *     F = (a.y*b.z - a.z*b.y,  a.z*b.x - a.x*b.z,  a.x*b.y - a.y*b.x)
 *   Area weighting: the face's own length is its weight.
 *   GROUPS: `groups` is optional, n_vertices uint32 each < n_vertices; vertices with equal values form one group, NULL = every vertex is
 *   its own group.  All members of a group receive the same normal: a UV seam (positions duplicated, texture coordinates not) stays
 *   smooth, and a hard edge stays hard where the caller puts the duplicates in different groups.
 *   VERTEX NORMAL: let F_1 .. F_k be the faces with at least one corner in the vertex's group, each taken once, in ascending face order.
 *     S = ((...((0 + F_1) + F_2) ...) + F_k)      per component, starting from +0
 *     d = (S.x*S.x + S.y*S.y) + S.z*S.z
 *     if d > 0 and d < +inf:  inv = 1.0f / sqrtf(d);  n' = (S.x*inv, S.y*inv, S.z*inv)
 *     else:                   n' = S
 *   A vertex whose group has no face keeps its normal bits.  Position and texture coordinate are never touched.  NaN and infinity go
 *   through as the arithmetic says.
 *
 * glz_renderer_add_normals returns the set's id (>= 0).  The face list and a row of face numbers per vertex are made once, on the host,
 * and uploaded; the caller's groups are not kept.  The rule then runs once, and the scene does what
 * glz_renderer_update_vertices(GLZ_GEOMETRY_REFIT) does after its upload, over the set's range: idle first, accumulation restarts, every
 * device follows.  FROM THEN ON the set's normals on the device are THE NORMAL RULE of the device's current positions: every
 * glz_renderer_update_vertices, glz_renderer_pose_skins and glz_renderer_animate whose written span overlaps the set's REACH (the lowest to
 * the highest vertex index of any corner of its faces) runs the rule over the whole set after its own writes and before the derivatives
 * and the one update of the structure, whose span is the union of the written span and the recomputed sets' ranges;
 * glz_geometry_update_info.update_ms includes the rule's kernels.  An update outside every reach runs nothing more than it did.
 * WARNING: a set over a skinned or morphed range REPLACES the normal THE SKINNING RULE transforms or THE MORPH RULE blends (and the
 * normals glz_renderer_update_vertices is given) in that range: the scene then equals one created with
 * glz_host_vertex_normals(glz_host_skin(...)), not with glz_host_skin(...) alone.  The previous-vertex buffers of read_motion* /
 * reproject* need positions only and are not touched by the rule.
 * Sets belong to the SCENE object, as skins and morphs do: ids count up and are never reused, every device of set_devices gets them, and a
 * set may overlap skins and morphs freely -- but no other set.  GLZ_E_ARG (nothing changes): a null pointer, n_vertices == 0, a range past
 * the vertex count, a group label >= n_vertices, a range overlapping another set.
 * glz_renderer_remove_normals frees a set; the vertices stay as they are, and later updates write what they wrote before the set was
 * there.  GLZ_E_ARG: no such set. */
typedef struct glz_normals {
  uint32_t        first_vertex, n_vertices;
  const uint32_t* groups;   /* n_vertices labels, each < n_vertices; NULL: every vertex is its own group */
} glz_normals;
int glz_renderer_add_normals(glz_renderer*, const glz_normals*);
int glz_renderer_remove_normals(glz_renderer*, int id);
/* raytracer.rs:328-356: the texture array changed under the same materials and lights (the reference re-binds the
 * textures it shares with the realtime viewer); accumulation is NOT restarted, like the reference. */
int glz_renderer_refresh_binded_textures(glz_renderer*, const glz_texture* textures, uint32_t n_textures);
int glz_renderer_wait_idle(glz_renderer*);                                /* raytracer.rs:328-340 */
/* Integrator::steps_per_sample()  raytracer.rs:78-85 (PATH_TRACE -> the configured depth) */
uint32_t glz_renderer_steps_per_sample(const glz_renderer*);

/* draw(spp, callback) -> RgbaImage   raytracer.rs:615-687.  Resets accumulation, runs
 * spp * steps_per_sample launches, calls `cb(user)` once per spp on the caller's thread
 * (raytracer.rs:651-653), writes W*H RGBA8 sRGB pixels (alpha 255) to rgba8_out (may be NULL). */
int glz_renderer_draw(glz_renderer*, size_t spp, void (*cb)(void*), void* user, uint8_t* rgba8_out);

/* draw_frame(): ONE launch = one path segment per pixel  (raytracer.rs:369-613), the unit the
 * interactive viewer drives.  `n` launches are enqueued; accumulation continues unless
 * glz_renderer_restart() was called (request_new_frame). */
int glz_renderer_restart(glz_renderer*);
int glz_renderer_step(glz_renderer*, uint32_t n_launches);
int glz_renderer_read_rgba8(glz_renderer*, uint8_t* rgba8_out); /* blit out32->out8 + export, memory.rs:269-483 */

/* ---- build-defined extensions (no reference counterpart) ---------------- */
int glz_renderer_set_seed(glz_renderer*, uint64_t seed);    /* replaces Xoshiro128PlusPlus::from_entropy, raytracer.rs:779 */
int glz_renderer_set_depth(glz_renderer*, uint32_t pt_steps);/* replaces const PT_STEPS = 6, raytrace_structures.rs:87 */
/* Texture level of detail.  The reference's samplers have LINEAR mip filtering and mip chains (generated by
 * LINEAR blits at upload when the file brings none, vulkan/scene.rs:1012-1263), but its ray-tracing stages call texture() with
 * the implicit level, which outside fragment shaders is level 0: GLZ_LOD_BASE (the default) reproduces that bit for bit.
 * GLZ_LOD_RAY_CONES picks the level per hit from the ray's footprint (cone width carried along the path, triangle texture /
 * world area ratio, angle of incidence) and blends the two nearest levels; the chain is built on the first launch that needs it.
 * GLZ_LOD_RAY_CONES_ANISO adds what the sampler's anisotropy (scene.rs:716-749: enabled at the device's maximum) does in the raster
 * viewer: the footprint is the cone's width across and width / |cos| along the ray's projection onto the surface; up to 16
 * trilinear probes along that axis, each at the level of its share of it, averaged.
 * Restarts accumulation. */
#define GLZ_LOD_BASE 0
#define GLZ_LOD_RAY_CONES 1
#define GLZ_LOD_RAY_CONES_ANISO 2
int glz_renderer_set_texture_lod(glz_renderer*, int mode);
/* cumulative image (xyz = sum of rgb radiance, w = launch count; path_trace.rgen:119-133),
 * W*H*4 floats, row-major, to host memory. */
int glz_renderer_read_hdr(glz_renderer*, float* rgba32f_out);
/* result image (`out32`: cumulative.xyz*exposure/w at the pixel's last update, path_trace.rgen:131-132) */
int glz_renderer_read_result(glz_renderer*, float* rgba32f_out);
/* per-launch host constants the draw loop will use for launch `i` after a restart:
 * seed (u32) and WorkScheduler pixel offset (raytracer.rs:486-489, :1168-1206). */
int glz_renderer_launch_constants(glz_renderer*, uint32_t launch, uint32_t* seed, float offset[2]);
/* camera push constants: camera2world then screen2camera, column-major (raytracer.rs:1098-1120) */
int glz_renderer_push_constants(glz_renderer*, float out32[32]);

/* ---- post: first-hit feature buffers and the edge-aware denoiser (build-defined; the reference has neither) ------------- */
/* The first-hit pass: ONE primary ray per pixel through the pixel centre (offset 0.5, 0.5; no jitter, no seed), tmin 1e-4, for the whole
 * frame on the renderer's own device whatever the tile partition, chains or set_devices say.  It is recomputed on every request (it
 * costs less than one render launch) and touches neither the accumulators nor the path state.  Two row-major RGBA32F planes:
 *   GLZ_AOV_NORMAL_DEPTH     xyz = the shading normal the shading code builds its frame from (interpolated, normal-mapped, object ->
 *                            world), normalised and turned towards the camera; (0,0,0) for a miss or a degenerate normal.
 *                            w = the hit distance t, +inf for a miss.
 *   GLZ_AOV_ALBEDO_INSTANCE  rgb = texture(diffuse).rgb * diffuse_mul for Lambert and Uber materials (texture level 0 always), (1,1,1)
 *                            for the other families and for a miss.  w = the bits of the hit's RTInstance index, 0xFFFFFFFF for a miss. */
#define GLZ_AOV_NORMAL_DEPTH 0
#define GLZ_AOV_ALBEDO_INSTANCE 1
int glz_renderer_read_aov(glz_renderer*, int which, float* rgba32f_out);   /* runs the first-hit pass; W*H*4 floats, row-major */

/* Which surface the two planes describe (glz_renderer_read_aov, glz_renderer_read_denoised; glaze-cli --guides).  The default is the first
 * hit, as above.  GLZ_GUIDE_THROUGH_SPECULAR follows the ray the path itself would follow through the materials it flags specular (Mirror
 * and Glass, RTMaterial::is_specular) to the first vertex that is not: inside a planar mirror and behind a window the filter then sees
 * the reflected / refracted geometry and texture instead of one featureless surface.  THE SPECIFICATION (B = max_bounces,
 * 1 <= B <= GLZ_GUIDE_MAX_BOUNCES):
 *   THE CHAIN.  Segment 0 is the centre ray of the first-hit pass: camera_ray at (1/2, 1/2), tmin 1e-4, tmax inf.  Vertex k is the closest
 *     hit of segment k (the render kernels' tracer, alpha tests inline).  If vertex k's material has is_specular != 0 and k < B, segment
 *     k + 1 has origin = point and direction = wiW, tmin 1e-4, tmax inf, with point and wiW formed as the shading kernel forms them for the
 *     path: barycentric point, object -> world; normal map, make_frame(dpdu, ns), woW = -direction of segment k; bsdf_sample at texture
 *     level 0 -- the same operations in the same order, hence the same bits -- with xi = (0, 0, 1 - 2^-24): Mirror ignores xi, Glass takes
 *     the transmitted branch unless its Fresnel term is 1 (total internal reflection), with the refraction as the renderer computes it
 *     (Q7): the guide follows what the renderer shows.  The chain ends at vertex k when bsdf_sample returns pdf 0 or a direction that is not
 *     finite.
 *   THE REPORTING VERTEX r is the first vertex whose material is not specular.  If a segment j >= 1 misses, if the cap is reached (vertex B
 *     is specular) or if the chain ends as above, r is the last vertex that was hit.  If segment 0 misses the pixel is a miss as above.
 *   THE PLANES.  GLZ_AOV_NORMAL_DEPTH: xyz = the normal rule above at vertex r, turned against the direction of segment r;
 *     w = ((t_0 + t_1) + ...) + t_r in binary32, in that order: the distance along the unfolded path, continuous across a planar mirror.
 *     GLZ_AOV_ALBEDO_INSTANCE: rgb = the albedo rule above at vertex r ((1,1,1) when r is itself specular), w = the instance of vertex r.
 *     A pixel whose first hit is not specular has the same bits in both modes.
 * The setting is held by the root renderer only (like the denoiser's parameters: the post stage runs on its device), and changing it does
 * not restart accumulation.  max_bounces is ignored with GLZ_GUIDE_FIRST_HIT.  GLZ_E_ARG, with nothing changed: a null renderer, an
 * unknown mode, max_bounces outside 1 .. GLZ_GUIDE_MAX_BOUNCES with GLZ_GUIDE_THROUGH_SPECULAR. */
#define GLZ_GUIDE_FIRST_HIT 0
#define GLZ_GUIDE_THROUGH_SPECULAR 1
#define GLZ_GUIDE_MAX_BOUNCES 8
int glz_renderer_set_guide_mode(glz_renderer*, int mode, uint32_t max_bounces);
int glz_renderer_guide_mode(glz_renderer*, uint32_t* max_bounces_out);   /* returns the mode (or a negative status); max_bounces_out may be NULL */

/* The denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on the albedo-demodulated result image, guided by the two
 * planes above.  Its edge-stopping functions are rational (1 / (1 + r^2)) so that the whole filter is + - * /, comparisons and selects:
 * host and device compute it bit for bit alike.  THE SPECIFICATION (every operation in binary32, no contraction, in this order;
 * "finite(v)" = |v| <= FLT_MAX, false for NaN; c = result, n / z = normal / depth, a = albedo):
 *   A(p)   = per channel a(p) > eps_albedo ? a(p) : eps_albedo
 *   i_0(p) = c(p).rgb / A(p);  every frame's .w = c(p).w
 *   hit(p) = finite(z(p))
 *   g(p)   = (gx, gy), for a hit p and per axis: f = z(next) - z(p), b = z(p) - z(previous), each usable if the neighbour is inside the
 *            image and the difference is finite; both usable: |b| < |f| ? b : f; one usable: that one; none: 0
 *   pass k = 0 .. iterations - 1, s = 2^k, sigma_k = sigma_color * (1 / 2^k), S = sigma_k * sigma_k:
 *     P = i_k(p) if all three channels are finite, else (0,0,0);   NP = (P.x*P.x + P.y*P.y) + P.z*P.z
 *     taps q = p + s (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner, summed in that order; a tap is DROPPED when q is outside the
 *     image, when a channel of Q = i_k(q) is not finite, when hit(q) != hit(p), or when its weight W is not > 0:
 *       centre tap (dx = dy = 0): W = 1
 *       D = Q - P;  d2 = (D.x*D.x + D.y*D.y) + D.z*D.z;  NQ = (Q.x*Q.x + Q.y*Q.y) + Q.z*Q.z
 *       cn = S * ((NP + NQ) + eps_color);  cd = cn + d2                      (the colour weight Wc = cn / cd = 1 / (1 + d2 / cn))
 *       misses: W = cn / cd.   hits:
 *         Wn = (n(p).x*n(q).x + n(p).y*n(q).y) + n(p).z*n(q).z, 0 unless > 0, then squared normal_power_log2 times
 *         ax = float(s*dx) * gx;  ay = float(s*dy) * gy
 *         a  = (z(q) - z(p)) - (ax + ay);  b = sigma_depth * ((|ax| + |ay|) + eps_depth * z(p))
 *         zn = b*b;  zd = zn + a*a                                           (the depth weight Wz = zn / zd = 1 / (1 + (a/b)^2))
 *         W  = (Wn * (cn * zn)) / (cd * zd)                                  (Wn Wz Wc as ONE quotient)
 *       hw = (h[dy] * h[dx]) * W with h = (1/16, 1/4, 3/8, 1/4, 1/16);   sw += hw;   sum.c += hw * Q.c per channel
 *     i_{k+1}(p) = sum / sw per channel if sw > 0, else i_k(p) unchanged (a non-finite pixel without a usable neighbour stays as it is)
 *   out(p).rgb = i_K(p) * A(p)
 * Defaults (glz_renderer_set_denoise(r, NULL)): iterations 5, sigma_color 4, sigma_depth 1, normal_power_log2 6 (cos^64), eps_albedo
 * 1/256, eps_depth 1e-3, eps_color 1e-8.  GLZ_E_ARG: iterations outside 1 .. GLZ_DENOISE_MAX_ITERATIONS, a sigma that is not finite and
 * positive, normal_power_log2 above GLZ_DENOISE_MAX_NORMAL_POWER_LOG2 (31: after 31 squarings every float below 1 has become 0, more
 * would only be a longer loop in every tap).  The epsilons are taken as they are.  Beware of eps_depth = 0: where the depth plane is
 * constant around a hit (a wall that faces the camera) b is 0, W is 0 / 0 and every tap but the centre is dropped -- the filter is the
 * identity there.  Products of very large depths and radiances can overflow cd * zd with the same effect. */
#define GLZ_DENOISE_MAX_ITERATIONS 8
#define GLZ_DENOISE_MAX_NORMAL_POWER_LOG2 31
typedef struct glz_denoise_params {
  uint32_t iterations;
  float sigma_color, sigma_depth;
  uint32_t normal_power_log2;
  float eps_albedo, eps_depth, eps_color;
} glz_denoise_params;
int glz_renderer_set_denoise(glz_renderer*, const glz_denoise_params*);   /* NULL = defaults; does not restart accumulation */
/* Either output may be NULL.  Flushes pending shadow rays and gathers like glz_renderer_read_result (chains, devices of set_devices),
 * runs the first-hit pass and the filter on the renderer's own device; rgba8_out is the filtered image through the sRGB quantiser of
 * glz_renderer_read_rgba8.  GLZ_E_ARG under glz_renderer_set_partition(world > 1): the frame is not in this process. */
int glz_renderer_read_denoised(glz_renderer*, float* rgba32f_out, uint8_t* rgba8_out);

/* Firefly rejection: an opt-in stage of the post stage that clamps a hit pixel whose demodulated brightness stands far above a robust mean
 * of its neighbours'.  The a-trous filter above cannot do this: its colour weight is relative (Wc >= 16/18 in pass 0 at the default
 * sigma_color however bright the neighbour is), so a firefly enters every pixel within reach at almost full weight.  The rule edits no
 * render kernel and is, like the filter, + - * /, comparisons and selects: host and device compute it bit for bit alike.
 * THE SPECIFICATION (every operation in binary32, no contraction, in this order; finite, A, i_0 and hit as the filter defines them, with
 * the eps_albedo of the denoise parameters in force):
 *   L(p)      = (i_0(p).x + i_0(p).y) + i_0(p).z
 *   usable(q) = q inside the image, hit(q), all three channels of i_0(q) finite
 *   p is a CANDIDATE iff usable(p).  Every other pixel (misses, non-finite pixels) passes through unchanged and is nobody's neighbour.
 *   window: q = p + (dx, dy), dy = -radius .. radius outer, dx = -radius .. radius inner, q != p, usable(q);  m = their number
 *   if m <= trim: unchanged
 *   M  = the (trim + 1)-th largest L(q) of the window, counted with multiplicity
 *   mu = (sum over the window, in window order, of (L(q) < M ? L(q) : M)) / float(m)      (a winsorised mean: no cancellation, ties are
 *                                                                                          harmless)
 *   T  = ratio * mu
 *   if T >= 0 and L(p) > T:  f = T / L(p);  i_0'(p).rgb = (i_0(p).x * f, i_0(p).y * f, i_0(p).z * f)    else i_0'(p) = i_0(p)
 *   .w passes through
 * All reads come from i_0 and all writes go to another frame: no pixel sees a neighbour that has already been clamped.  Misses (the sky,
 * the sun seen directly) are noise-free in this renderer and are never touched.
 * With the rejection enabled glz_renderer_read_denoised runs the filter's passes on i_0' instead of i_0; glz_renderer_read_despeckled
 * returns i_0' * A with no filter pass at all.
 * Defaults (params NULL): radius 2, trim 2, ratio 8.  GLZ_E_ARG, before anything is launched and with nothing changed: radius other than 1
 * or 2, trim above GLZ_DESPECKLE_MAX_TRIM (3), a ratio that is not finite or below 1.
 * KNOWN COSTS.  It is a biased estimator: it removes energy.  A lit pixel whose window holds at most `trim` lit neighbours goes black
 * (M = 0, hence T = 0).  An isolated one-pixel emitter is treated as a firefly.  A cluster of more than `trim` adjacent fireflies
 * survives -- counted as the rule counts, q != p: a firefly with more than `trim` fireflies among its window's neighbours, for then M is a
 * firefly's L (T is at least (trim + 1) * ratio / m of it).  With up to `trim` of them around it, it is brought down like a lone one. */
#define GLZ_DESPECKLE_MAX_TRIM 3
typedef struct glz_despeckle_params {
  uint32_t radius, trim;
  float ratio;
} glz_despeckle_params;
/* params NULL = defaults; enabled != 0 puts the rejection ahead of the filter in glz_renderer_read_denoised.  The default state is
 * disabled.  Held by the root renderer only, like the denoiser's parameters; does not restart accumulation and touches neither the path
 * state nor the accumulators. */
int glz_renderer_set_despeckle(glz_renderer*, int enabled, const glz_despeckle_params*);
int glz_renderer_despeckle(glz_renderer*, glz_despeckle_params* out);   /* returns the enabled flag (or a negative status); out may be NULL */
/* The result image through the rejection alone, with the parameters in force whatever the enabled flag says: gathers and runs the
 * first-hit pass (or the guide chain of the mode in force) like glz_renderer_read_denoised, then i_0' * A; no filter pass runs.  Either
 * output may be NULL; rgba8_out goes through the sRGB quantiser of glz_renderer_read_rgba8.  GLZ_E_ARG under
 * glz_renderer_set_partition(world > 1). */
int glz_renderer_read_despeckled(glz_renderer*, float* rgba32f_out, uint8_t* rgba8_out);

/* Motion vectors and history reprojection: the geometric half of a temporal filter.  Where was the surface point a pixel shows on screen in
 * the previous frame, and does the previous pixel there still show the same surface?  Stateless: the caller keeps the previous camera, the
 * previous transforms and the previous frames; nothing here blends, keeps a history, restarts accumulation or touches the path state or
 * the accumulators.  Everything runs on the renderer's own device over the whole frame, as glz_renderer_read_aov does (so it also works
 * under glz_renderer_set_partition and glz_renderer_set_devices).  THE SPECIFICATION (every operation in binary32, no contraction, in this
 * order; finite as the filter defines it; sqrt correctly rounded; floor exact):
 *   PROJECTION CONSTANTS (glz_host_project_constants, the forward twin of glz_host_push_constants): out32[0..16) = world2camera =
 *     look_at_rh(camera), out32[16..32) = camera2screen = projection(camera, w, h) with m[5] negated -- the two matrices whose inverses
 *     the push constants are -- column-major, formed in binary64 and rounded to binary32 once.  Nothing is inverted.
 *   project_point(M = world2camera, S = camera2screen, camera type, w, h, P) -> (fx, fy, z):
 *     Pc.r = ((M[r]*P.x + M[4+r]*P.y) + M[8+r]*P.z) + M[12+r]                                             r = 0, 1, 2
 *     perspective:  d = -Pc.z;  ndc.r = (((S[r]*Pc.x + S[4+r]*Pc.y) + S[8+r]*Pc.z) + S[12+r]) / d  (r = 0, 1);
 *                   z = sqrt((Pc.x*Pc.x + Pc.y*Pc.y) + Pc.z*Pc.z)
 *     orthographic: ndc = (Pc.x, Pc.y);  z = -Pc.z;  d counts as positive     (camera_ray's orthographic branch: the ray starts at
 *                   camera2world * (ndc.x, ndc.y, 0, 1) and runs along the view axis -- the projection's scale is not applied, Q18 kept)
 *     fx = ((ndc.x + 1) * 0.5) * w;   fy = ((ndc.y + 1) * 0.5) * h
 *     (fx, fy) is the continuous pixel position (pixel centres at + 1/2, row-major, y down), the inverse of camera_ray's
 *     ndc = -1 + 2 (pixel / size); z is the distance at which camera_ray of that camera through (fx, fy) reaches P.
 *     INVALID -- the result is (0, 0, +inf) -- unless d > 0, finite(z), z > 0, finite(fx) and finite(fy).  (An intermediate beyond
 *     FLT_MAX is an infinity in binary32 and makes the point invalid: coordinates of 1e30 overflow Pc.x*Pc.x.)
 *   THE MOTION PLANE (glz_renderer_read_motion): one row-major float4 per pixel p = (px, py), describing the first hit of the centre ray
 *     (segment 0 of the first-hit pass, whatever glz_renderer_set_guide_mode says):
 *     b0 = 1 - u - v;  P_obj = (v0*b0 + v1*u) + v2*v per component, from the hit triangle's object-space positions
 *     P' = prev_o2w[transform id] applied to P_obj: per row r, m[r]*x + m[4+r]*y + m[8+r]*z + m[12+r] summed left to right.  The transform
 *       id is the hit instance's.  prev_transforms == NULL means "the instances did not move": the scene's own object -> world matrices.
 *       Nothing is skipped for an identity transform.
 *     (fx, fy, z') = project_point(previous camera, P')
 *     plane = (fx - (float(px) + 0.5), fy - (float(py) + 0.5), z', the first hit's instance bits)
 *     a miss: (0, 0, +inf, 0xFFFFFFFF);   an invalid projection: (0, 0, +inf, instance bits)
 *     With previous vertices (glz_previous_state::vertices, glz_renderer_read_motion_from): let (i0, i1, i2) be the hit triangle's three
 *       entries of the index buffer, in index-buffer order -- the order of the shading record and of the barycentrics.
 *       vk' = the position of vertices[ik - first_vertex] if first_vertex <= ik < first_vertex + n_vertices, else the current position of
 *       vertex ik
 *       P_obj' = (v0'*b0 + v1'*u) + v2'*v per component, the same expression in the same order as P_obj
 *       P' = prev_o2w[transform id] applied to P_obj'
 *       Only positions are read: normals and texture coordinates of the array are ignored.  The instance bits, the miss rule and the
 *       invalid rule do not change.
 *   THE REPROJECTION RULE (glz_renderer_reproject, glz_host_reproject), per pixel p, from the motion plane m and three PREVIOUS frames:
 *     the colour c (any RGBA32F image), aov0 = (normal, depth) and aov1 = (albedo, instance bits), both from GLZ_GUIDE_FIRST_HIT:
 *     z' = m.z not finite: out = (0, 0, 0, 0).  Otherwise
 *     q = p + (m.x, m.y) -- the pixel centre moved by the motion, in pixel-corner coordinates ((px + 1/2) + m.x - 1/2) -- taken apart exactly:
 *     x0 = px + floor(m.x), y0 = py + floor(m.y) (integers), a = (m.x - floor(m.x), m.y - floor(m.y)) (exact in binary32): no rounding
 *     of q's hundreds of pixels reaches the weights
 *     four taps t = (x0 + dx, y0 + dy), dy = 0, 1 outer, dx = 0, 1 inner, with W = (dx ? a.x : 1 - a.x) * (dy ? a.y : 1 - a.y)
 *     a tap is ACCEPTED iff it lies inside the frame (a motion that is not finite has no tap inside), the bits of aov1(t).w equal the bits
 *     of m.w, the three colour channels of c(t) are finite, and |zh - z'| <= depth_tolerance * z' (false when a side is NaN), where
 *       zh = z(t) + (gx * (a.x - float(dx)) + gy * (a.y - float(dy)))                    (a - d = q - t)
 *     is the tap's depth carried to q by the filter's own first-order model: (gx, gy) = g(t) of the filter's specification above, taken
 *     on the previous depth plane at the tap.
 *     sw = sum of W, sum.c = sum of W * c(t).c over the accepted taps, in tap order, each starting from 0
 *     out = (sum.x / sw, sum.y / sw, sum.z / sw, sw) if sw > 0, else (0, 0, 0, 0).   out.w is a confidence in 0 .. 1.
 *     There is no normal test: carrying a normal into the previous frame needs the previous transform's inverse.
 * Default (params NULL): depth_tolerance 1/64.  GLZ_E_ARG, before anything is launched and with nothing changed: a null renderer, camera,
 * frame or output; a non-NULL prev_transforms whose count is not the scene's (with NULL the count is ignored); a depth_tolerance that is
 * not finite and positive. */
typedef struct glz_reproject_params {
  float depth_tolerance;
} glz_reproject_params;
/* All frames are row-major W*H*4 floats in host memory. */
int glz_renderer_read_motion(glz_renderer*, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms, float* out);
/* The first-hit trace, the motion plane, then the rule on the three uploaded frames. */
int glz_renderer_reproject(glz_renderer*, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms,
                           const float* prev_color, const float* prev_aov0, const float* prev_aov1, const glz_reproject_params* params_or_null, float* out);
/* The same two calls for a scene whose meshes deform (glz_renderer_update_vertices): the previous state with the previous VERTICES in it,
 * which the caller keeps like the previous camera and transforms -- nothing is kept here between calls.  The two calls above are the case
 * vertices == NULL, and with it these give their planes bit for bit.  The array is uploaded for the call and released with it; only its
 * positions are read.  GLZ_E_ARG, before anything is launched and with nothing changed: a null renderer, state, camera or output; a
 * non-NULL transforms whose count is not the scene's; non-NULL vertices with n_vertices == 0 or with a range that reaches past the
 * scene's vertex count (with NULL vertices, first_vertex and n_vertices are ignored, as n_transforms is with NULL transforms); for
 * glz_renderer_reproject_from the frame and parameter checks of glz_renderer_reproject. */
typedef struct glz_previous_state {
  const glz_camera*    camera;         /* required */
  const glz_transform* transforms;     /* NULL = the instances did not move (the scene's own); else n_transforms = the scene's count */
  uint32_t             n_transforms;
  const glz_vertex*    vertices;       /* NULL = the meshes did not deform; else the PREVIOUS contents of the scene's vertices */
  uint32_t             first_vertex;   /*   [first_vertex, first_vertex + n_vertices), exactly the range update_vertices takes */
  uint32_t             n_vertices;
} glz_previous_state;
int glz_renderer_read_motion_from(glz_renderer*, const glz_previous_state*, float* out);
int glz_renderer_reproject_from(glz_renderer*, const glz_previous_state*, const float* prev_color, const float* prev_aov0,
                                const float* prev_aov1, const glz_reproject_params* params_or_null, float* out);
/* The same for a scene whose meshes are POSED (glz_renderer_pose_skins): the previous vertices never visit the host.  The state's
 * vertices must be NULL; the buffer the motion kernel reads is filled on the device instead -- the span from the lowest to the highest
 * vertex of the named skins is copied from the scene's current vertices (a gap between skins holds current values), then the skinning
 * rule runs with the PREVIOUS bones, once per skin.  The planes equal, bit for bit, those of read_motion_from / reproject_from given the
 * vertices glz_host_skin makes of the previous bones over that span.  GLZ_E_ARG (nothing launched, nothing changed): the checks of
 * read_motion_from / reproject_from, non-NULL state->vertices, and the pose checks of glz_renderer_pose_skins. */
int glz_renderer_read_motion_posed(glz_renderer*, const glz_previous_state*, const glz_pose* prev_poses, uint32_t n_prev_poses, float* out);
int glz_renderer_reproject_posed(glz_renderer*, const glz_previous_state*, const glz_pose* prev_poses, uint32_t n_prev_poses, const float* prev_color,
                                 const float* prev_aov0, const float* prev_aov1, const glz_reproject_params* params_or_null, float* out);
/* The same for a scene that is ANIMATED (glz_renderer_animate): state->vertices must be NULL; the previous-vertex buffer is the current
 * vertices of the span copied device to device, then every named morph and skin run with the PREVIOUS weights and bones, as
 * glz_renderer_animate runs them.  The planes equal, bit for bit, those of read_motion_from / reproject_from given the vertices the host
 * references make of the previous animation over that span.  GLZ_E_ARG (nothing launched, nothing changed): the checks of
 * read_motion_from / reproject_from, non-NULL state->vertices, and the animation checks of glz_renderer_animate. */
int glz_renderer_read_motion_animated(glz_renderer*, const glz_previous_state*, const glz_animation* prev, float* out);
int glz_renderer_reproject_animated(glz_renderer*, const glz_previous_state*, const glz_animation* prev, const float* prev_color, const float* prev_aov0,
                                    const float* prev_aov1, const glz_reproject_params* params_or_null, float* out);

/* Multi-GPU (one process per GPU): this renderer owns the 64x64-pixel tiles t with
 * t % world == rank; other pixels stay zero.  The exchange of the HDR accumulator itself is done
 * by the caller (RCCL through torch.distributed or rccl directly) on the device buffers below. */
int glz_renderer_set_partition(glz_renderer*, uint32_t rank, uint32_t world);
/* Scatters the owned tiles of the cumulative image (which = 0) or of the result image `out32`
 * (which = 1) into a caller-provided DEVICE buffer of W*H*4 floats, zero elsewhere, on the instance
 * stream (synchronised before returning): the operand of ncclReduce(sum).  Tiles are disjoint, so
 * the sum over ranks is bit-identical to a single-GPU render. */
int glz_renderer_export_device(glz_renderer*, int which, void* dev_rgba32f);
/* The same exchange with 1 / world of the bytes: a rank's tiles ONLY, tile-major (64x64 pixels of 4 floats per tile, local
 * tile j = global tile rank + j * world), glz_renderer_packed_pixels(r, rank, world) pixels -- the operand of an ncclSend /
 * gather to rank 0, which puts every received buffer in its place of a full frame with glz_renderer_scatter_packed (nothing
 * but those tiles is written; rank 0's own tiles come from glz_renderer_export_device).  Device pointers; synchronised
 * before returning. */
uint64_t glz_renderer_packed_pixels(glz_renderer*, uint32_t rank, uint32_t world);
int glz_renderer_export_packed(glz_renderer*, int which, void* dev_packed_rgba32f);
int glz_renderer_scatter_packed(glz_renderer*, uint32_t rank, uint32_t world, const void* dev_packed_rgba32f, void* dev_frame_rgba32f);
/* The receiving side of a gather in ONE call: `dev_packed_rgba32f` holds the packed tiles of ranks 0 .. world - 1 one after the other,
 * `stride_pixels` pixels apart (what a gather into one buffer leaves; >= glz_renderer_packed_pixels(r, 0, world)); every rank's tiles go
 * to their place in the frame -- world small kernels on the instance stream, ONE synchronisation (rank 0's own tiles included: the
 * frame needs no glz_renderer_export_device first, the tiles of all ranks cover it). */
int glz_renderer_scatter_packed_all(glz_renderer*, uint32_t world, const void* dev_packed_rgba32f, uint64_t stride_pixels, void* dev_frame_rgba32f);
/* Concurrent chains: the tiles of this process advance as `n` independent launch sequences on `n` HIP streams (0 = automatic:
 * one chain while the rank owns a million pixels, two down to 400 k, three below).  Pixels never interact, so the image does not depend on n; with a small
 * tile share per GPU the chains fill the machine while the longest rays of a launch finish. */
int glz_renderer_set_chains(glz_renderer*, uint32_t n);
/* How a launch (one path segment per pixel, draw_frame) reaches the device.  GLZ_LAUNCH_TWO_KERNELS: k_trace + k_shade per launch over
 * all pixels -- throughput, the full frame.  GLZ_LAUNCH_PATH: every wave carries its 64 pixels through the launches of a batch
 * (closest hits -> shadow rays of the launch before -> shading) inside one persistent kernel, no grid-wide boundary between launches
 * -- latency, a small tile share per GPU (a 1080p frame over 8 GPUs); flattened scenes, and only while the work counters are off.
 * GLZ_LAUNCH_AUTO (default): by the pixels this device owns.  The image does not depend on the mode.  glz_renderer_launch_mode
 * returns the mode in force (never AUTO). */
#define GLZ_LAUNCH_AUTO 0
#define GLZ_LAUNCH_TWO_KERNELS 1
#define GLZ_LAUNCH_PATH 2
int glz_renderer_set_launch_mode(glz_renderer*, int mode);
int glz_renderer_launch_mode(glz_renderer*);
/* Which nodes the two-kernel mode's traversal walks (build-defined; the reference's structure is the driver's, acceleration.rs:319-345):
 * 4 = the 64-byte 4-wide nodes (k_trace), 8 = the 128-byte 8-wide nodes of the same hierarchy (k_trace8; flattened scenes, and only
 * while the work counters are off -- the counted walk is the 4-wide one), 0 (default) = automatic, which is 4: the 8-wide walk visits
 * 31 % fewer nodes and measured slower at every tile share, it is kept as a tested option.  The image does not
 * depend on it.  glz_renderer_node_width returns the width in force. */
int glz_renderer_set_node_width(glz_renderer*, int width);
int glz_renderer_node_width(glz_renderer*);
/* Multi-GPU inside ONE process (what a Rust glaze-cli bound to this library uses for `--devices`; the reference drives exactly one
 * VkPhysicalDevice, lib/src/vulkan/device.rs:252-321): hip_devices[0] must be the renderer's own device (glz_instance_device);
 * every further device gets a stream, a replica of the scene (upload + BVH build on that device), a renderer for the 64x64 tiles
 * t % n == i and a host thread that enqueues its launches.  All setters, step / draw and scene updates apply to every device;
 * every read-back (read_hdr / read_result / read_rgba8 / draw's image / export_device) first brings the other devices' tiles
 * onto hip_devices[0] over RCCL / xGMI (one communicator per device from ncclCommInitAll, all calls of one exchange in one
 * ncclGroup): by default every device ncclSends its packed tiles (1 / n of the frame) and device 0 ncclRecvs and scatters
 * them; with GLAZE_MULTI_EXCHANGE=reduce in the environment at this call, one ncclReduce(sum, float) of the zero-padded
 * RGBA32F frame per device; with GLAZE_MULTI_EXCHANGE=peer no RCCL at all: one hipMemcpyPeerAsync of the packed tiles per device,
 * ordered into device 0's stream by events (never chosen by the library itself).  The tiles are disjoint, so the image is
 * bit-identical to a one-device render.  n = 1 returns to one
 * device; after a failure the renderer is a one-device renderer again.  Not combinable with glz_renderer_set_partition (one process per GPU).  RCCL is loaded on first use
 * (librccl.so.1); GLZ_E_DEVICE when it is missing.  With GLAZE_MULTI_LOOPBACK=1 in the environment the list may name ONE
 * device n times (tests on a one-GPU machine: same sharding, threads and replicas, the tiles meet without RCCL). */
int glz_renderer_set_devices(glz_renderer*, const int* hip_devices, int n);
int glz_renderer_device_count(glz_renderer*);   /* devices this renderer spans (1 unless set_devices succeeded with more) */
int glz_renderer_device_scene_info(glz_renderer*, int i, glz_scene_info* out);   /* the scene replica device i renders (0 = the renderer's own) */
int glz_rccl_version(void);                     /* ncclGetVersion() of the RCCL this library loads (> 0), or a negative status */
/* Tonemaps a full-frame DEVICE result image (e.g. the reduced one on rank 0) to RGBA8 sRGB host memory. */
int glz_renderer_tonemap_device(glz_renderer*, const void* dev_result_rgba32f, uint8_t* rgba8_out);

/* ---- measurement ------------------------------------------------------------------------ */
typedef struct glz_render_stats {
  uint64_t launches;        /* launches since the last restart */
  uint64_t samples;         /* owned pixels x launches */
  double   render_ms;       /* device time of those launches (hipEvent, instance stream) */
  double   trace_closest_ms, shade_ms, trace_shadow_ms, other_ms; /* per-kernel-class device time: k_trace, k_shade, stand-alone shadow passes, k_path (GLZ_LAUNCH_PATH) */
  uint64_t closest_rays, shadow_rays;
  /* traversal work counters (only filled when counting is enabled, slows rendering down) */
  uint64_t closest_nodes, closest_tris, shadow_nodes, shadow_tris, hits;
  uint64_t fresh_paths;     /* closest rays that were new camera rays (bounce 0) */
  /* tracer phase occupancy, counting build only: {node rounds, node lanes, leaf rounds, leaf lanes, refills, refilled lanes} x {closest, shadow} */
  uint64_t phase[12];
  /* shading-side work, counting build only: texture fetches that read memory (bilinear: four texels each; 1 x 1 textures live in
   * their descriptor and are not counted) and their texel bytes (16 per RGBA fetch, 4 per gray one) -- of which alpha_tex_bytes in
   * the traversal kernel's alpha tests --, light samples of omni / sun / area lights (one 112-byte RTLight each) and of the sky
   * (a binary search of the marginal table, two values of the conditional tables, one texel fetch, counted above) */
  uint64_t tex_fetches, tex_bytes, alpha_tex_bytes, light_samples, sky_samples;
} glz_render_stats;
/* bit 0: traversal work counters (slower kernels); bit 1: per-kernel hipEvent timing (on by default) */
int glz_renderer_enable_counters(glz_renderer*, int flags);
int glz_renderer_get_stats(glz_renderer*, glz_render_stats* out);

/* ---- debug / parity hooks (used by tests; run on the device, no CPU fallback) -------------- */
/* closest hit of n rays: t (inf = miss), world triangle id (instance-major), barycentric u,v */
int glz_debug_trace_closest(glz_scene*, const float* origins3, const float* dirs3, uint64_t n, float tmin,
                            float* t_out, uint32_t* tri_out, uint32_t* inst_out, float* u_out, float* v_out);
int glz_debug_trace_any(glz_scene*, const float* origins3, const float* dirs3, const float* tmax, uint64_t n,
                        float tmin, uint8_t* hit_out);
/* Derivatives buffer (normal, dpdu, dpdv as 3 x vec4 per object-space triangle), generate_derivatives.comp */
int64_t glz_debug_read_derivatives(glz_scene*, float* out12, int64_t cap_triangles);
/* Device-side sky tables / RT arrays as uploaded (for parity with the oracle's host prep) */
int64_t glz_debug_read_rt_materials(glz_scene*, void* out, int64_t cap_bytes); /* 208-byte RTMaterial records */
int64_t glz_debug_read_rt_lights(glz_scene*, void* out, int64_t cap_bytes);    /* 112-byte RTLight records */
int64_t glz_debug_read_sky(glz_scene*, float* out, int64_t cap_floats);        /* RTSky(36 f32) | header(4) | marginal arrays */
/* BVH as traversed by the kernels: 64-byte quantised 4-wide nodes (returns the node count) and 48-byte leaf
 * triangles in leaf order (n_world_triangles of them; a leaf is one triangle or two adjacent ones, bit 30 of the
 * first one's last word says which, and leaf links name the first); see DESIGN.md for the layouts. */
int64_t glz_debug_read_bvh(glz_scene*, void* nodes_out, int64_t cap_nodes, void* tris_out, int64_t cap_tris);
/* The same hierarchy as 128-byte 8-wide nodes (what the tracer of a small tile share walks; glz_scene_info::bvh_nodes8 of them, flattened
 * builds only): child k's box words at [3k .. 3k+2], its link at [24 + k], leaf links name the first triangle slot as above. */
int64_t glz_debug_read_bvh8(glz_scene*, void* nodes_out, int64_t cap_nodes);
/* The 64-byte per-leaf records the tracers read, as they are on the device (returns their count; a two-level scene's are its meshes' concatenated) */
int64_t glz_debug_read_leaf_records(glz_scene*, void* out, int64_t cap_records);

/* 192-byte TlasInstance records of a two-level scene in the top level's leaf order (returns the byte count; 0 for a flattened scene) */
int64_t glz_debug_read_tlas_instances(glz_scene*, void* out, int64_t cap_bytes);
/* Instance boxes of a two-level scene under its current transforms, 4 floats each (xyz, 0): on_device 0 = the host rule, 1 = the
 * device kernel update_transforms uses.  budget: point transforms before the remaining instances take their mesh box's corners
 * (0 = the library's own).  Returns the instance count (0 for a flattened scene); lo4 / hi4 take 4 x that many floats.  With both
 * NULL only the count is returned and nothing runs. */
int64_t glz_debug_instance_boxes(glz_scene*, int on_device, uint64_t budget, float* lo4, float* hi4);
/* device-event time in ms of the instance-box kernels the last time they ran for this scene (an update, or glz_debug_instance_boxes
 * on the device), the item upload and read-back excluded; -1 if they never ran */
float glz_debug_box_kernel_ms(glz_scene*);
/* one level of a scene texture's mip chain as the device holds it (level 0 = the texture; builds the chain if needed): returns the
 * byte count (0 past the last level), writes up to cap bytes and the level's dimensions */
int64_t glz_debug_read_texture_level(glz_scene*, uint32_t texture, uint32_t level, uint8_t* out, int64_t cap, uint32_t* width, uint32_t* height);
/* k_tonemap (the out32 -> RGBA8 sRGB blit, raytracer.rs:576-584) on n host pixels of RGBA32F: upload, kernel, read back */
/* the two references above on the device, on arrays the caller supplies: the parity hooks (kernel_ms_out, may be NULL: k_reproject alone
 * between device events) */
int glz_debug_project_points(glz_instance*, const glz_camera* camera, uint32_t width, uint32_t height, const float* points3, uint64_t n, float* out3);
int glz_debug_reproject(glz_instance*, uint32_t w, uint32_t h, const float* motion, const float* prev_color, const float* prev_aov0, const float* prev_aov1,
                        const glz_reproject_params* params_or_null, float* out, float* kernel_ms_out);
/* glz_renderer_read_motion's pass without the read-back: the device-event time of k_motion alone, in milliseconds */
int glz_debug_motion_timing(glz_renderer*, const glz_camera* prev_camera, const glz_transform* prev_transforms, uint32_t n_prev_transforms, float* kernel_ms_out);
/* the same for glz_renderer_read_motion_from: k_motion_deform alone when the state has vertices */
int glz_debug_motion_timing_from(glz_renderer*, const glz_previous_state*, float* kernel_ms_out);
/* k_skin alone on one skin of the scene, into a scratch buffer (the scene is untouched): the device-event time of `reps` launches after
 * one that is not timed, divided by reps.  The pose is checked as glz_renderer_pose_skins checks it.  A skin in
 * GLZ_SKIN_DUAL_QUATERNION mode is timed with its own kernel, k_skin_dq (and k_morph_skin_dq below, at 32 bytes a bone). */
int glz_debug_skin_timing(glz_renderer*, const glz_pose* pose, uint32_t reps, float* kernel_ms_out);
/* k_clip_bones alone for ONE play (checked as glz_renderer_play checks it): the bone table as the device holds it afterwards, in the
 * skin's current blend layout -- rows_out: 3 x n_bones float4 for a linear skin (row after row of each bone), 2 x n_bones in
 * GLZ_SKIN_DUAL_QUATERNION mode -- and, for a clip with a weight track, its n_targets weights (weights_out may be NULL).  No vertex is
 * written: with it, a failing vertex test says which stage failed. */
int glz_debug_clip_bones(glz_renderer*, const glz_play* play, float* rows_out, float* weights_out);
/* k_clip_bones alone, one launch for all the plays, timed as glz_debug_skin_timing times k_skin; the plays are checked as
 * glz_renderer_play checks them, the table of (clip, k0, k1, u) goes up once, outside the timed span. */
int glz_debug_clip_timing(glz_renderer*, const glz_play* plays, uint32_t n_plays, uint32_t reps, float* kernel_ms_out);
/* The morph kernels alone, into a scratch buffer (the scene is untouched), timed as glz_debug_skin_timing times k_skin.  `one` names one
 * morph and no pose -- k_morph on it, from the skin's bind pose if it is attached -- or one attached morph and its skin's pose --
 * k_morph_skin.  bytes_out (may be NULL): the bytes one launch moves by the layout's own count -- per vertex 32 in, 32 out and 4 of row
 * length, 8 a slice, 32 an entry that is not padding, 4 a target; fused, also 24 a vertex of joints and weights and 48 a bone. */
int glz_debug_morph_timing(glz_renderer*, const glz_animation* one, uint32_t reps, float* kernel_ms_out, uint64_t* bytes_out);
/* The two kernels of one normal set alone, timed as glz_debug_skin_timing times k_skin: k_face_vectors into a scratch buffer of face
 * vectors, then k_vertex_normals from it into a scratch copy of the set's vertices (the scene is untouched).  ms_out[0] / bytes_out[0]: the
 * face kernel, [1]: the vertex kernel.  bytes_out (may be NULL): per face 12 of indices, 3 x 16 gathered, 16 out; per vertex 4 of row
 * length, 4 + 16 a row entry that is not padding, 8 a slice, and 32 in + 12 out for a vertex that has a face. */
int glz_debug_normals_timing(glz_renderer*, int id, uint32_t reps, float ms_out[2], uint64_t bytes_out[2]);
int glz_debug_tonemap(glz_instance*, const float* rgba32f, uint64_t n_pixels, uint8_t* rgba8_out);
/* The kernels' texture sampler on n coordinates uv2[2i], uv2[2i+1] of a scene texture, RGBA out: level 0 (texture2d) when
 * footprint4 is NULL, else the level of detail of footprint4[4i..4i+3] = (lod_base, du, dv, taps in 1..16) (texture2d_lod, after
 * building the mip chain).  The scene's own texel pool and descriptors. */
int glz_debug_sample_texture(glz_scene*, uint32_t texture, const float* uv2, const float* footprint4_or_null, uint64_t n, float* rgba_out);
/* include/glz_detmath.h on the device: fn 0 sin, 1 cos, 2 acos, 3 atan2(y, x), 4 log2, 5 floor of n values (y only for atan2) */
int glz_debug_detmath(glz_instance*, int fn, const float* x, const float* y, float* out, uint64_t n);
/* The kernels' colour-to-spectrum conversion (device/shading.h: from_surface_color, or from_illuminant_color when illuminant != 0)
 * of n colours rgb3[3i..3i+2]; out16 takes 16 floats per colour */
int glz_debug_color_to_spec(glz_instance*, int illuminant, const float* rgb3, uint64_t n, float* out16);
/* The kernels' shading routines one call at a time, n elements each (device/shading.h: bsdf_eval, bsdf_sample, sample_light followed by
 * light_emission).  The surface point is set up as the shading kernel sets it up (material scalars, the material's textures at level 0
 * for the ONE pair uv2 of the call), except the frame: frame9 = s, t, n, stored as given, NULL = (1,0,0), (0,1,0), (0,0,1).  value16 /
 * emission16 take 16 floats per element.  Outputs start as zeros and keep them where a routine returns early (pdf 0).  A material id or
 * light index (RTLight records: an area light has one per instance) out of range is GLZ_E_ARG. */
int glz_debug_bsdf_value(glz_scene*, uint32_t material_id, const float* wo3, const float* wi3, const float* uv2, const float* rand1,
                         const float* frame9_or_null, uint64_t n, float* value16_out, float* pdf_out);
int glz_debug_bsdf_sample(glz_scene*, uint32_t material_id, const float* wo3, const float* uv2, const float* rand3, const float* frame9_or_null,
                          uint64_t n, float* wi3_out, float* value16_out, float* pdf_out);
int glz_debug_light_sample(glz_scene*, uint32_t light_index, const float* pos3, const float* rand3, uint64_t n, float scene_radius,
                           float* wi3_out, float* dist_out, float* pdf_out, float* emission16_out);
/* For the two BSDF hooks above: gives one material's record metal spectra of the caller's (ior = n, ior2abs2 = n^2 + k^2, 16 bins each; any
 * floats, NaN and zeros included -- pairs no built-in metal has), and derives the shading tables again as a material update does, the
 * glz_host_conductor_finite flag included.  For a scene no renderer is rendering; the next glz_renderer_update_materials_and_lights puts
 * the material's own metal back.  A material id out of range is GLZ_E_ARG. */
int glz_debug_scene_set_spectra(glz_scene*, uint32_t material_id, const float ior[16], const float ior2abs2[16]);

/* The device filter of glz_denoise_params on host arrays (w*h*4 floats each, row-major): upload, kernels, read back.  params NULL = defaults. */
int glz_debug_denoise(glz_instance*, uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1,
                      const glz_denoise_params*, float* out);
/* The device side of glz_host_despeckle on host arrays: upload, k_demodulate, k_despeckle (and the filter's passes with with_filter), read
 * back.  kernel_ms_out (may be NULL) receives the device-event time of k_despeckle alone, in milliseconds. */
int glz_debug_despeckle(glz_instance*, uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1,
                        const glz_despeckle_params*, const glz_denoise_params*, int with_filter, float* out, float* kernel_ms_out);
/* One run of the post stages of this renderer between device events (hipEvent on the instance stream), in ms: ms_out[0] the first-hit
 * trace kernel, [1] its attribute kernel, [2] the demodulation, [3 + k] a-trous pass k (entries past the configured iterations are 0).
 * Gathers the result image first, like glz_renderer_read_denoised; nothing is read back. */
#define GLZ_POST_TIMING_SLOTS (3 + GLZ_DENOISE_MAX_ITERATIONS)
int glz_debug_post_timing(glz_renderer*, float ms_out[GLZ_POST_TIMING_SLOTS]);
/* camera_ray() of every pixel at one sub-pixel offset, on the device: W*H*3 floats each, row-major (the first-hit pass uses 0.5, 0.5) */
int glz_debug_camera_rays(glz_renderer*, float off_x, float off_y, float* origins3, float* dirs3);

/* The rays of segment `segment` of every pixel's guide chain under the mode and cap in force (0 = the camera rays of the first-hit pass):
 * W*H*3 floats each and W*H bytes, row-major.  alive[p] = 1 where pixel p's chain has that segment -- every pixel for segment 0; for
 * segment k >= 1 the pixels whose vertices 0 .. k - 1 were all hit and specular and went on, with k <= max_bounces in
 * GLZ_GUIDE_THROUGH_SPECULAR, none in GLZ_GUIDE_FIRST_HIT -- and its origin and direction are 0 where it has not. */
int glz_debug_guide_chain(glz_renderer*, uint32_t segment, float* origins3, float* dirs3, uint8_t* alive);

/* First contact with RCCL on this machine: a one-rank communicator on the instance's device (ncclCommInitAll), one
 * ncclReduce(sum, float) of n_floats values on the instance's stream, result compared bit for bit with the input, communicator
 * destroyed.  version_out (may be NULL) receives ncclGetVersion(). */
int glz_debug_rccl_selftest(glz_instance*, uint64_t n_floats, int* version_out);

/* ---- host logic, callable without a device (used by the CPU test-suite and by bindings) ------ */
/* seed + pixel offset of launch `launch` after a restart, for renderer seed `seed`
 * (rng.gen::<u32>() + WorkScheduler::next(), raytracer.rs:486-489, :1168-1206) */
int glz_host_launch_constants(uint64_t seed, uint32_t launch, uint32_t* seed_out, float offset[2]);
/* build_push_constants (raytracer.rs:1098-1120): camera2world then screen2camera, column-major */
int glz_host_push_constants(const glz_camera* camera, uint32_t width, uint32_t height, float out32[32]);
/* rank owning each pixel under glz_renderer_set_partition(., world): 64x64 tiles, tile t -> t % world */
int glz_host_tile_owner(uint32_t width, uint32_t height, uint32_t world, uint16_t* owner_out);
/* launch chains a renderer of this size and partition runs with (chains = 0: the automatic choice of glz_renderer_set_chains), and the
 * chain rendering each pixel of rank `rank` (0xFFFF for pixels of other ranks): chain s of S owns tiles t with t % (world*S) == rank + s*world */
int glz_host_chain_owner(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint32_t chains, uint16_t* owner_out);
/* the host side of GLZ_BVH_SAH on its own (no GPU): binary hierarchy over n >= 2 leaf boxes (box_lo / box_hi: 4 floats per leaf,
 * xyz used).  children_out[2 * i], [2 * i + 1] for inner node i < n - 1: link >= 0 inner node, < 0 ~leaf; parent_out[i] for
 * inner node i (root 0: -1), parent_out[n - 1 + l] for leaf l. */
/* the 8-bit sRGB quantiser of read_rgba8 / draw (the reference's R8G8B8A8_SRGB blit, raytracer.rs:576-584): c encodes to
 * #{k in 1..255 : c >= thresholds_out[k]}; thresholds_out[0] = 0 */
int glz_host_srgb8_thresholds(float thresholds_out[256]);
/* the per-row table a sky sample reads once its row is found, as scene creation builds it from the sky's marginal values and conditional
 * integrals (n rows each): pairs_out[2 y] = marginal_values[y], pairs_out[2 y + 1] = conditional_integrals[y] -- the same floats, interleaved */
int glz_host_sky_row_pairs(const float* marginal_values, const float* conditional_integrals, uint64_t n, float* pairs_out);
/* the bracket table scene creation makes of the sky's marginal cdf (`size` entries) for the kernels' row search: 257 entries, entry b the
 * index at which the full search's bisection ends for xi = b / 256; 0xFFFF in every entry (the fall-back table: searches take the whole
 * cdf) when the cdf has a descent or a NaN, or 65 535 entries or more */
int glz_host_sky_bracket_table(const float* cdf, uint64_t size, uint16_t* table_out);
/* the kernels' row search on the host, for n values xi: the full bisection (bracket_or_null null) or the one that starts inside the
 * bracket of xi (a table of glz_host_sky_bracket_table for this cdf; GLZ_E_ARG for one that leaves it); xi outside [0, 1), a NaN and the
 * fall-back table take the full search.  sample_out[i] = (row + position inside the row's step) / size, offset_out[i] = the row */
int glz_host_sky_cdf_search(const float* cdf, uint64_t size, const uint16_t* bracket_or_null, const float* xi, uint64_t n, float* sample_out, uint32_t* offset_out);
/* the texel index the sampler gives integer coordinate i in a REPEAT texture of n >= 1 texels: the non-negative remainder, taken as
 * i & (n - 1) when n is a power of two and through i % n otherwise, as the kernels do */
int glz_host_texel_wrap(const int32_t* i, uint64_t count, int32_t n, int32_t* index_out);
/* the flag scene creation and material updates give a pair of metal spectra (ior = n, ior2abs2 = n^2 + k^2, 16 bins each): *flag_out = 1
 * when the conductor Fresnel term of the pair is finite in every bin for every cosine |c| <= 2 -- both are finite and at most 2^60 in
 * magnitude, and the minima over |c| <= 2 of a + 2nc + c^2 and of a c^2 + 2nc + 1 are at least 2^-10 (|a| + 4|n| + 5), in double
 * precision -- else 0.  An Uber hit of a flagged pair whose metalness is zero and whose cosine is within |c| <= 2 skips the term: its
 * product with the metalness is a zero, and the result has the same bits. */
int glz_host_conductor_finite(const float ior[16], const float ior2abs2[16], int* flag_out);
/* the pair of built-in metal `metal` (glz_material::metal, below GLZ_METAL_COUNT of glz_tables.h) as a material's record carries it */
int glz_host_metal_spectra(uint32_t metal, float ior_out[16], float ior2abs2_out[16]);
/* the size check of scene creation (glz_instance_set_bvh_builder: "Size limit") on counts given by the caller, nothing built or
 * allocated: 4-wide nodes, 8-wide nodes, leaf records, instance records, lanes of the largest persistent grid, spilt stack words per
 * lane.  GLZ_OK when every table stays below 2^32 bytes, else GLZ_E_INVALID_DATA with the message scene creation fails with. */
int glz_host_traversal_offsets_fit(uint64_t n_nodes, uint64_t n_nodes8, uint64_t n_leaves, uint64_t n_instances, uint64_t grid_lanes,
                                   uint64_t overflow_depth);
/* one level of the mip chain the library generates for a texture that brings only level 0 (mipchain.h: LINEAR-blit rule); returns the
 * byte count of that level (0 past the last), writes up to cap bytes */
int64_t glz_host_mip_level(const glz_texture* texture, uint32_t level, uint8_t* out, int64_t cap, uint32_t* width, uint32_t* height);
int glz_host_build_sah(uint32_t n, const float* box_lo, const float* box_hi, int32_t* children_out, int32_t* parent_out);
/* the filter of glz_denoise_params on the host, no device: the reference the device kernels are compared with bit for bit.
 * result / aov0 / aov1 / out: w*h*4 floats, row-major; out must not overlap an input.  params NULL = defaults. */
int glz_host_denoise(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1,
                     const glz_denoise_params*, float* out);
/* the firefly rejection of glz_despeckle_params on the host, no device (either params NULL = defaults).  with_filter = 0: out = i_0' * A,
 * and only eps_albedo of the denoise parameters is used (the other fields are not read, and not checked).  with_filter != 0: all of them
 * must be valid, and the filter's passes run on i_0' -- the composition
 * glz_renderer_read_denoised equals bit for bit when the rejection is enabled. */
int glz_host_despeckle(uint32_t w, uint32_t h, const float* result, const float* aov0, const float* aov1,
                       const glz_despeckle_params*, const glz_denoise_params*, int with_filter, float* out);
/* the host rule of glz_debug_instance_boxes on a scene description (no device): a mesh's box is the min / max of its vertices here.
 * One box per instance that names an existing mesh, in instance order; returns their count (both outputs NULL: the count alone). */
/* The references of the motion / reprojection specification above, no device.  project_constants: out32 as specified.  project_points:
 * n points (3 floats each) -> (fx, fy, z) each.  reproject: the rule on host arrays (params NULL = defaults). */
int glz_host_project_constants(const glz_camera* camera, uint32_t width, uint32_t height, float out32[32]);
int glz_host_project_points(const glz_camera* camera, uint32_t width, uint32_t height, const float* points3, uint64_t n, float* out3);
int glz_host_reproject(uint32_t w, uint32_t h, const float* motion, const float* prev_color, const float* prev_aov0, const float* prev_aov1,
                       const glz_reproject_params* params_or_null, float* out);
int64_t glz_host_instance_boxes(const glz_scene_desc* desc, uint64_t budget, float* lo4, float* hi4);
/* THE SKINNING RULE (glz_renderer_add_skin) on host arrays, no device: the reference k_skin is compared with bit for bit.  bind / out: n
 * vertices (out may be bind itself); joints, weights: 4 per vertex; bones: n_bones matrices.  GLZ_E_ARG: a null pointer with n > 0,
 * n_bones == 0, a joint >= n_bones. */
int glz_host_skin(const glz_vertex* bind, const uint16_t* joints, const float* weights, uint64_t n, const glz_transform* bones, uint32_t n_bones,
                  glz_vertex* out);
/* THE DUAL-QUATERNION RULE on host arrays, no device: the reference k_skin_dq is compared with bit for bit.  glz_host_skin_dq: the
 * arguments and the refusals of glz_host_skin.  glz_host_bone_dual_quats: the rule's bone conversion alone, n matrices -> 8 floats a
 * bone, (x, y, z, w) then (dx, dy, dz, dw); GLZ_E_ARG: a null pointer with n > 0. */
int glz_host_skin_dq(const glz_vertex* bind, const uint16_t* joints, const float* weights, uint64_t n, const glz_transform* bones, uint32_t n_bones,
                     glz_vertex* out);
int glz_host_bone_dual_quats(const glz_transform* bones, uint32_t n, float* out8);
/* THE CLIP RULE on host arrays, no device: the reference k_clip_bones is compared with bit for bit.  The structs of
 * glz_renderer_add_skeleton / glz_renderer_add_clip, their `skin` / `skeleton` ids ignored and n_bones the skeleton's own.  bones_out:
 * n_bones matrices B[b], column-major, with the fourth row (0, 0, 0, 1) -- what glz_renderer_pose_skins takes.  weights_out: the
 * clip's n_targets lerped weights; may be NULL, and is not written for a clip without a weight track.  GLZ_E_ARG: a null pointer,
 * n_bones == 0, a parent that is neither -1 nor below its bone, n_keys == 0, times not finite or not strictly ascending, null
 * translations or rotations, a weight track with n_targets == 0, a non-finite time. */
typedef glz_skeleton glz_skeleton_desc;
typedef glz_clip glz_clip_desc;
int glz_host_clip_bones(const glz_skeleton_desc* skeleton, const glz_clip_desc* clip, float time, glz_transform* bones_out, float* weights_out);
/* THE MORPH RULE (glz_renderer_add_morph) on host arrays, no device: the reference k_morph is compared with bit for bit; it runs through
 * the same layout packer as glz_renderer_add_morph.  base / out: n vertices (out may be base itself); targets, n_targets: as glz_morph
 * has them, over n vertices; weights: n_targets.  GLZ_E_ARG: a null pointer with n > 0, and what glz_renderer_add_morph refuses of a
 * morph's targets. */
int glz_host_morph(const glz_vertex* base, uint64_t n, const glz_morph_target* targets, uint32_t n_targets, const float* weights, glz_vertex* out);
/* THE NORMAL RULE (glz_renderer_add_normals) on host arrays, no device: the reference k_face_vectors and k_vertex_normals are compared
 * with bit for bit; it runs through the same layout packer as glz_renderer_add_normals.  vertices, indices, meshes: a scene's, whole;
 * first_vertex, n, groups_or_null: as glz_normals has them; out: n vertices, the range's own with the rule's normals (out may be
 * vertices + first_vertex itself).  GLZ_E_ARG: a null pointer, what glz_renderer_add_normals refuses of a set, a mesh whose index range
 * is past n_indices, an index >= n_vertices. */
int glz_host_vertex_normals(const glz_vertex* vertices, uint64_t n_vertices, const uint32_t* indices, uint64_t n_indices, const glz_mesh* meshes, uint64_t n_meshes,
                            uint32_t first_vertex, uint32_t n, const uint32_t* groups_or_null, glz_vertex* out);
/* Group labels for glz_normals.groups by welding: groups_out[i] = the lowest index j of the n vertices whose three position words and
 * three normal words are bit-equal to i's (so -0 is not +0).  A convenience for callers: the library itself never welds.  GLZ_E_ARG: a
 * null pointer with n > 0, n > 2^32 - 1. */
int glz_host_weld_groups(const glz_vertex* vertices, uint64_t n, uint32_t* groups_out);

#ifdef __cplusplus
}
#endif
#endif /* GLAZE_ABI_H */
